// float32 engine (streaming kernels + the driver of the LDS-resident path)
#include "lds_engine.h"

EngineBase* mg_make_engine_f32(mgadmm_solver* s) { return new LdsEngine(s); }
