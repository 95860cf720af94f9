// MG_HD: marks a function of a plain C++ header callable from host and device code when a HIP compiler reads the header,
// and is empty otherwise (the CPU checks under tests/cpu compile the same headers with g++).
#pragma once
#ifdef __HIPCC__
#define MG_HD __host__ __device__
#else
#define MG_HD
#endif
