"""GPU check that two builds of the library give the same BITS.  A child process per library (MGADMM_LIB), each one GPU step
under its own `timeout`, runs on the cfg2 tables
  - the LDS path: a cfg2-shaped solve (B=512, 6 ADMM iterations, float32), a masked DGLR solve and a DGTV solve;
  - the streaming path (path='stream', B=64, 3 iterations), float32 and float64: ablation None and masked DGLR, one solve that
    records the CG coefficients, one with a shared param_schedule, one resumed from the state the plain solve returned, and
    two_loops with 2 outer x 2 inner iterations;
  - cfg3 (N = 10000, B = 512, float32: the tiled and fused streaming kernels), 3 iterations;
  - a float64 line-graph instance of width 3 on the cfg2 tables, 12 samples under the band tables of intervals 1, 2, 3;
and the parent compares x, the exported state, the residual history, the CG counts and the recorded coefficients.
      python tools/ab_bitwise.py <lib A> <lib B>"""
import os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 420

CHILD = r'''
import os, sys
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "mixed-graph-admm_amd"))
import numpy as np, torch
import bench, mgadmm
dev = torch.device("cuda", 0)
out = {}
n, B, cl, dl, info, desc = bench.build_problem("cfg2")

def product(abl, dtype=torch.float32, **kw):
    blk = mgadmm.ADMM_algorithm({"n_nodes": n}, info, use_kNN=True, k=4, u_sigma=50, d_sigma=50, tables=(cl, dl), device=dev,
                                compute_dtype=dtype, ablation=abl, **kw)
    blk.check_stop = False
    return blk

def inputs(B, masked, dtype=torch.float32):
    y = bench.synth_y(n, B, 24 if masked else 12, seed=3, offset=0, device=dev)
    m = None
    if masked:
        m = (torch.rand(y.shape, generator=torch.Generator().manual_seed(4)) > 0.3).float().to(dev)
        y = y * m
    return y.to(dtype), m            # (the results come back in y's dtype)

def keep(name, blk, x=None):
    for k, v in blk.state.items():
        if v is not None:
            out[name + ".state." + k] = v.cpu().numpy()
    if x is not None:
        out[name + ".x"] = x.cpu().numpy()
        out[name + ".pres"] = np.array(blk.p_res_list); out[name + ".dres"] = np.array(blk.d_res_list)
    for nm in ("CG_iter_x", "CG_iter_zu", "CG_iter_zd"):
        if getattr(blk, nm):
            out[name + "." + nm] = torch.stack(getattr(blk, nm)).numpy()
    for nm in ("alpha_x", "beta_x", "alpha_zu", "beta_zu", "alpha_zd", "beta_zd"):
        if getattr(blk, nm):
            out[name + "." + nm] = np.stack([np.asarray(v) for v in getattr(blk, nm)])

for name, abl, masked in (("pred", "None", False), ("mask_dglr", "DGLR", True), ("pred_dgtv", "DGTV", False)):
    blk = product(abl)
    blk.max_ADMM_iter = 6
    y, m = inputs(512, masked)
    keep(name, blk, blk.solve(y, mask=m)[0])
    blk.close()

for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
    for abl, masked in (("None", False), ("DGLR", True)):
        name = f"stream_{tag}_{abl}"
        blk = product(abl, dtype, path="stream", record_cg_coeffs=False)
        blk.max_ADMM_iter = 3
        y, m = inputs(64, masked, dtype)
        keep(name, blk, blk.solve(y, mask=m)[0])
        first = dict(blk.state)
        blk._reset_history()
        keep(name + "_resumed", blk, blk.solve(y, mask=m, warm_start=first)[0])
        if abl == "None":
            blk._reset_history()
            ramp = {"rho": info["rho"] * np.array([1.0, 1.5, 2.0]), "rho_u": info["rho_u"] * np.array([1.0, 0.75, 0.5])}
            keep(name + "_schedule", blk, blk.solve(y, mask=m, param_schedule=ramp)[0])
            blk._reset_history()
            blk.record_cg_coeffs = True
            keep(name + "_record", blk, blk.solve(y, mask=m)[0])
            blk.record_cg_coeffs = False
        blk._reset_history()
        blk.max_ADMM_iter, blk.max_inner_iter = 2, 2
        blk.two_loops(y, mask=m)
        keep(name + "_two_loops", blk)
        blk.close()

n3, B3, cl3, dl3, info3, _ = bench.build_problem("cfg3")
blk = bench.make_solver(n3, cl3, dl3, info3, dev)
blk.max_ADMM_iter = 3
keep("cfg3", blk, blk.solve(bench.synth_y(n3, B3, 12, seed=1, offset=0, device=dev))[0])
blk.close()

blk = mgadmm.ADMM_algorithm({"n_nodes": n}, info, use_kNN=True, k=4, u_sigma=50, tables=(cl, dl), device=dev, compute_dtype=torch.float64,
                            use_line_graph=True, skip_connection=3, path="stream")
blk.check_stop, blk.max_ADMM_iter = False, 3
keep("band_f64", blk, blk.solve(inputs(12, False, torch.float64)[0], band_params={"skip": [1, 2, 3] * 4})[0])
blk.close()
np.savez(OUT, **out)
'''

def run(lib, out):
    env = dict(os.environ, MGADMM_LIB=os.path.abspath(lib))
    code = f"ROOT = {ROOT!r}\nOUT = {out!r}\n" + CHILD
    subprocess.check_call(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, "-c", code], env=env)

if __name__ == "__main__":
    import numpy as np
    a, b = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as tmp:
        fa, fb = os.path.join(tmp, "ab_a.npz"), os.path.join(tmp, "ab_b.npz")
        run(a, fa); run(b, fb)        # (a child that fails ends the script: nothing more is started)
        A, Bz = dict(np.load(fa)), dict(np.load(fb))
    assert sorted(A) == sorted(Bz), sorted(set(A) ^ set(Bz))
    bad = 0
    for k in A:
        same = A[k].shape == Bz[k].shape and np.array_equal(A[k], Bz[k], equal_nan=True)
        d = float(np.abs(A[k].astype(np.float64) - Bz[k].astype(np.float64)).max()) if not same and A[k].shape == Bz[k].shape else 0.0
        print(f"{k:40s} {'identical' if same else 'DIFFERENT max abs diff %.3e' % d}")
        bad += not same
    print("ALL IDENTICAL" if bad == 0 else f"{bad} arrays differ")
    sys.exit(1 if bad else 0)
