"""The whole-batch metrics of the LDS path in two launches per iteration (csrc/lds_metric_kernels.h: k_lds_metric_pass sums
x - x_old over slices of 64 samples, k_lds_metric_final forms delta_x_per_step and the whole-batch value of every metric),
on the helper stream of the CHUNKS schedule beside the next launches (single-wave workgroups) and, after the last chunk, on an
idle GPU (256-thread workgroups), against
  * the same library with MGADMM_LDS_ASYNC=0 (one stream, every pass in the idle shape): x, the exported state, every history
    list, delta_x_per_step, the per-sample sums and the CG counts, bit for bit;
  * the float64 oracle run on the whole batch: helpers.check_windows on every sample (x per sample 1e-5, per-sample lists
    rtol 1e-3 with the floor 1e-7 ||x||, CG counts +-1), the whole-batch lists at the same rtol and floor, and
    delta_x_per_step at rtol 1e-3 with a floor of its own (below).
Every leg is a child process (`python tests/lds_metric_pass_cases.py <case> <out.npz>`): the two switches are read when a
solver is created.

Cases: the g4 kNN table (N = 30, T = 24, the uniform TPG-8 instance), 7 iterations, B = 1, 63, 64, 65, 130 (below, at and
across the 64-sample slice of the pass, a ragged last slice) x MGADMM_LDS_CHUNK = 1, 3, 16 (one trip per launch, a ragged last
chunk, the whole solve in one chunk: every pass in the idle shape); and from lds_row_order_cases.py `aligned` (masked input,
N = 128) and `cfg2mask` (ablation 'DGTV', masked, the bench graph) in chunks of 3; and the pass cut into one or two workgroups
of 64, 256 and 512 threads (MGADMM_LDS_METRIC_SHAPE), B = 130 in chunks of 3, against the synchronous loop.

Floor of delta_x_per_step[t] = || mean_b (x - x_old)[b, t, :] ||: either float32 iterate carries a rounding error of 2^-24
relative per entry, so an entry of the mean of the differences is off by at most 2^-23 = 1.2e-7 times the entry of x, and
the norm over the nodes of one time step by 1.2e-7 times the norm of one sample's x at one time step.  Rounding errors of
B samples do not add up in a mean, so the floor is 1e-7 ||x_oracle|| / sqrt(B T): the floor of check_windows for one
(sample, time step) block instead of the whole array.
"""
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import lds_metric_pass_cases as mc
from lds_metric_pass_cases import CG_LISTS, LISTS

pytestmark = pytest.mark.gpu

HTOL = 1e-3            # helpers.check_windows: every history list


def _leg(case, tmp, asynchronous, chunk=None, shape=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MGADMM_LDS_")}
    env["MGADMM_LDS_ASYNC"] = "1" if asynchronous else "0"
    if chunk is not None:
        env["MGADMM_LDS_CHUNK"] = str(chunk)
    if shape is not None:
        env["MGADMM_LDS_METRIC_SHAPE"] = shape
    out = os.path.join(str(tmp), f"{case.replace(':', '_')}_{int(asynchronous)}_{chunk}_{shape}.npz")
    p = subprocess.run([sys.executable, "-s", mc.__file__, case, out], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def sync_leg(tmp_path_factory):
    """The MGADMM_LDS_ASYNC=0 leg of a case, solved once (no chunk length enters it)."""
    tmp = tmp_path_factory.mktemp("metric_pass_sync")
    return functools.lru_cache(maxsize=None)(lambda case: _leg(case, tmp, False))


@functools.lru_cache(maxsize=None)
def _g4_oracle(B):
    from helpers import make_oracle
    meta = mc.g4_meta()
    o = make_oracle(meta, "knn")
    xo = o.combined_loop(mc.g4_inputs(meta, B).astype(np.float64), n_iters=mc.G4_ITERS)
    return o, xo


def _rc_oracle(name):
    import lds_row_order_cases as rc
    import mgadmm
    from oracle import admm_oracle as orc
    c = rc.case(name)
    y, mask = rc.inputs(c)
    kw = dict(u_sigma=c["sigma"], d_sigma=c["sigma"]) if c["sigma"] else {}
    ref = mgadmm.ADMM_algorithm({"n_nodes": c["N"]}, c["info"], use_kNN=True, k=4, tables=c["tables"], ablation=c["abl"],
                                t_in=c["t_in"], T=c["T"], record_cg_coeffs=False, path="stream", **kw)    # (the weight tables)
    o = orc.OracleADMM(ref.connect_list.numpy(), ref.u_ew[0].numpy(), ref.d_ew[0].numpy(), c["info"], mode="knn", ablation=c["abl"],
                       t_in=c["t_in"], T=c["T"])
    ref.close()
    xo = o.combined_loop(y.astype(np.float64), mask=mask, n_iters=c["iters"])
    return o, xo, c["abl"]


def _same_bits(a, b, tag):
    assert str(a["instance"]) == str(b["instance"]), tag
    assert sorted(a) == sorted(b), tag
    for k in a:
        if k != "instance":
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{tag}: {k}")


def _against_oracle(tag, d, o, xo, abl="None"):
    from helpers import check_windows
    B, T = xo.shape[0], xo.shape[1]
    h = o.hist
    blk = types.SimpleNamespace(metrics_per_sample=d["mps"], **{k: [torch.from_numpy(v) for v in d[k]] for k in CG_LISTS})
    check_windows(tag, blk, torch.from_numpy(d["x"]), np.arange(B), o, xo, abl=abl, finite_termination_rule=True)
    floor = 1e-7 * float(np.linalg.norm(xo))
    n_it = len(h.p_res_list)
    assert d["dxps"].shape == (n_it, T)
    ref = np.array(h.delta_x_per_step)
    floor_t = floor / np.sqrt(B * T)
    err = np.abs(d["dxps"] - ref)
    print(f"[metric pass] {tag}: delta_x_per_step max abs err {err.max():.3e} (floor {floor_t:.3e}), max rel err {(err / np.maximum(ref, 1e-300)).max():.3e}, "
          f"smallest value {ref.min():.3e}")
    np.testing.assert_allclose(d["dxps"], ref, rtol=HTOL, atol=floor_t, err_msg=f"{tag} delta_x_per_step")
    for k, atol in (("p_res_list", floor), ("d_res_list", floor), ("x_shift_list", floor), ("recover_list", floor), ("GLR_list", 0.0),
                    ("DGTV_list", 0.0), ("DGLR_list", 0.0)):
        want = np.array(getattr(h, k), dtype=np.float64)
        assert d[k].shape == want.shape, (tag, k, d[k].shape, want.shape)
        if want.size:
            np.testing.assert_allclose(d[k], want, rtol=HTOL, atol=atol, err_msg=f"{tag} {k}")


@pytest.mark.parametrize("chunk", [1, 3, 16])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_metric_pass_equals_the_synchronous_loop_and_the_oracle(B, chunk, sync_leg, tmp_path):
    case = f"g4:{B}"
    ref = sync_leg(case)
    new = _leg(case, tmp_path, True, chunk)
    assert str(new["instance"]).startswith("k_admm_lds<8, false,"), new["instance"]      # the uniform TPG-8 instance
    assert new["dxps"].shape == (mc.G4_ITERS, 24) and np.isfinite(new["dxps"]).all()
    for k in LISTS:
        assert np.isfinite(new[k]).all(), k
    _same_bits(new, ref, f"g4 B={B} chunk={chunk}")
    o, xo = _g4_oracle(B)
    _against_oracle(f"g4 B={B} chunk={chunk}", new, o, xo)


@pytest.mark.parametrize("shape", ["64x1", "256x2", "512x1"])
def test_metric_pass_in_few_workgroups(shape, sync_leg, tmp_path):
    """MGADMM_LDS_METRIC_SHAPE=<threads>x<workgroups>: the pass beside a launch in that many workgroups, several tasks per
    thread (B = 130, N = 30: 540 tasks), and the final with that many threads (at most 256)."""
    ref = sync_leg("g4:130")
    new = _leg("g4:130", tmp_path, True, 3, shape)
    _same_bits(new, ref, f"g4 B=130 chunk=3 shape={shape}")


@pytest.mark.parametrize("name", ["aligned", "cfg2mask"])
def test_metric_pass_on_masked_input_and_dgtv(name, sync_leg, tmp_path):
    case = f"rc:{name}"
    ref = sync_leg(case)
    new = _leg(case, tmp_path, True, 3)
    _same_bits(new, ref, f"{name} chunk=3")
    o, xo, abl = _rc_oracle(name)
    _against_oracle(f"{name} chunk=3", new, o, xo, abl=abl)
