"""The smooth, sparse-phi cases of tests/prox_cases.py and its one-step audit, on the CPU oracle alone.

  1. reference conditions: on every case the oracle's 6 iterations are finite and, at the two audited iterations (index 1 and 5)
     on the audited windows, the prox really thresholds: the zero class holds >= 5 % of the entries of phi (t >= 1) at both,
     each of the three classes (zero / positive / negative) >= 5 % at one of them at least, and at most 1 % of the entries lie
     within the float32 E_phi of +-threshold (those the class check leaves out);
  2. the audit accepts the oracle: consecutive float64 states pass at eps = 2^-52, every entry, no class mismatch;
  3. the audit discriminates: the states rounded to float32 with the step recomputed in correctly rounded float32 pass at
     eps = 2^-23; each of four wrong steps (zero class returns s, sign dropped, threshold mu_d1 / rho_u, gamma updated with the
     old phi) fails;
  4. abs_ldr, the sparse |Ldr| of the bounds, equals the absolute value of the oracle's dense Ldr on the small cases.
"""
import numpy as np
import pytest

import prox_cases as pc


def _audits(c, eps, states=None):
    ref = pc.reference(c)
    st = ref["states"] if states is None else states
    w = pc.solver_weights(c, ref["idx"], eps)
    return [pc.audit_step(ref["o"], st[i], st[i + 1], eps, w) for i in pc.AUDIT_AT]


def test_case_table_covers_what_it_names():
    import lds_census as lc
    lds = [c for c in pc.CASES if c["path"] == "lds"]
    rows = {r["expect"]: r for r in lc.CENSUS}
    for c in lds:
        r = rows[c["expect"]]
        assert c["dtype"] == "f32" and c["abl"] in ("None", "DGLR")
        assert all(c[k] == r[k] for k in ("N", "T", "t_in", "kind", "indeg", "abl", "task", "B", "env")), c["name"]
    has = lambda f: any(f(c) for c in lds)
    assert has(lambda c: c["expect"].startswith("k_admm_lds<8,") and "true, " in c["expect"].split("5,")[-1] and c["kind"] == "uniform")
    assert has(lambda c: c["expect"].startswith("k_admm_lds<8,") and "false, " in c["expect"].split("5,")[-1] and c["kind"] == "uniform")
    assert has(lambda c: c["expect"].startswith("k_admm_lds<12, false, 640") and c["kind"] == "uniform" and not c["env"])
    assert has(lambda c: c["expect"].startswith("k_admm_lds<12, false, 1024") and c["N"] == 512 and lc.geometry(c)[3] == 0)
    assert has(lambda c: c["kind"] == "knnpad" and c["task"] == "mask")
    assert has(lambda c: c["kind"] == "physical" and c["abl"] == "DGLR")
    assert has(lambda c: c["kind"] == "line1") and has(lambda c: c["kind"] == "line3" and c["abl"] == "DGLR")
    assert has(lambda c: c["env"].get("MGADMM_LDS_SB") == "1")
    pp = [c for c in lds if c["sample_params"]]
    assert len(pp) == 1 and pp[0]["B"] == 3 and pp[0]["sample_params"]["mu_d1"] == [1.0, 6.0, 12.0]
    r = np.sqrt(pp[0]["N"] / pp[0]["T"])
    np.testing.assert_allclose(pp[0]["sample_params"]["rho"], [r, 2 * r, 4 * r], rtol=1e-15)
    stream = [c for c in pc.CASES if c["path"] == "stream"]
    for c in stream:
        assert c["N"] <= 96 and c["N"] * c["T"] <= 2400 and c["B"] <= 5
    for kind in {c["kind"] for c in stream}:
        assert {(c["dtype"], c["reorder"]) for c in stream if c["kind"] == kind} == {("f32", None), ("f32", "cluster"), ("f64", None)}
    assert all(c["B"] <= 5 and len(pc.windows(c)) == 3 for c in pc.CASES)


def test_smooth_inputs():
    y, mask = pc.smooth_inputs(4, 24, 30, 12, "pred", seed=1)
    assert y.dtype == np.float64 and y.shape == (4, 12, 30, 1) and mask is None
    ym, m = pc.smooth_inputs(4, 24, 30, 12, "mask", seed=1)
    assert ym.shape == m.shape == (4, 24, 30, 1) and set(np.unique(m)) == {0.0, 1.0} and 0.5 < m.mean() < 0.7
    np.testing.assert_array_equal(ym[:, :12][m[:, :12] == 1], y[m[:, :12] == 1])          # the same x_true
    assert (ym[m == 0] == 0).all()
    x = ym[m == 1]
    assert 95 < x.min() and x.max() < 145
    d = np.diff(y, axis=1)                                   # smooth in time: steps of s_b + 0.4 sqrt(2) noise
    assert np.abs(d).max() < 5 and 0.4 < d.std() < 0.9


@pytest.mark.parametrize("c", pc.CASES, ids=pc.case_id)
def test_reference_conditions(c):
    ref = pc.reference(c)
    for _, o, x in ref["groups"]:
        assert np.isfinite(x).all() and len(o.hist.p_res_list) == pc.ITERS
        assert all(np.isfinite(v).all() for v in o.state.values())
        assert np.isfinite(np.array(o.hist.p_res_list)).all() and np.isfinite(np.array(o.hist.d_res_list)).all()
    aud = _audits(c, pc.F32_EPS)
    shares = np.array([a["shares"] for a in aud])
    print(f"\n[prox cases] {c['name']}: zero / positive / negative at iteration 1: " + "/".join(f"{v:.2f}" for v in shares[0])
          + ", at iteration 5: " + "/".join(f"{v:.2f}" for v in shares[1]) + f"; within E_phi of the threshold: {max(a['left_out'] for a in aud):.4f}")
    assert (shares[:, 0] >= pc.MIN_SHARE).all(), (c["name"], "zero class", shares)
    assert (shares.max(0) >= pc.MIN_SHARE).all(), (c["name"], "a class is empty at both iterations", shares)
    assert all(a["left_out"] <= pc.MAX_NEAR for a in aud), (c["name"], [a["left_out"] for a in aud])


@pytest.mark.parametrize("c", pc.CASES, ids=pc.case_id)
def test_audit_accepts_the_oracle(c):
    for i, a in zip(pc.AUDIT_AT, _audits(c, pc.F64_EPS)):
        assert not any(a["bad"].values()), (c["name"], i, a["bad"], a["ratio"])
        assert a["mismatch"] == 0 and a["left_out"] <= pc.MAX_NEAR, (c["name"], i, a["mismatch"], a["left_out"])
        assert set(a["ratio"]) == {"gamma_u"} | ({"phi", "gamma"} if c["abl"] in ("None", "DGLR") else set()) | ({"gamma_d"} if c["abl"] != "DGLR" else set())


@pytest.mark.parametrize("c", pc.CASES, ids=pc.case_id)
def test_audit_discriminates(c):
    ref = pc.reference(c)
    o, st = ref["o"], ref["states"]
    w = pc.solver_weights(c, ref["idx"], pc.F32_EPS)
    for i in pc.AUDIT_AT:
        A = {k: v.astype(np.float32).astype(np.float64) for k, v in st[i].items()}
        good = pc.audit_step(o, A, pc.step_in_float32(o, A, st[i + 1], w), pc.F32_EPS, w)
        assert pc.audit_ok(good), (c["name"], i, good["bad"], good["ratio"], good["mismatch"], good["left_out"])
        assert max(good["ratio"].values()) > 0.0                                  # (float32 really rounds)
        for v in pc.VARIANTS:
            bad = pc.audit_step(o, A, pc.step_in_float32(o, A, st[i + 1], w, variant=v), pc.F32_EPS, w)
            assert not pc.audit_ok(bad), (c["name"], i, v)
            assert bad["bad"]["gamma_u"] == 0 and bad["bad"].get("gamma_d", 0) == 0            # (those steps are right)
    # ... and a wrong gamma_u / gamma_d: the other one's penalty (3 r for 2 r and the reverse)
    i = pc.AUDIT_AT[0]
    A = {k: v.astype(np.float32).astype(np.float64) for k, v in st[i].items()}
    for k, other in (("rho_u", "rho_d"),) + ((("rho_d", "rho_u"),) if c["abl"] != "DGLR" else ()):
        w2 = dict(w, **{k: w[other]})
        bad = pc.audit_step(o, A, pc.step_in_float32(o, A, st[i + 1], w2), pc.F32_EPS, w)
        assert bad["bad"]["gamma" + k[3:]] > 0, (c["name"], k)


@pytest.mark.parametrize("c", [c for c in pc.CASES if c["path"] == "stream" and c["dtype"] == "f64"], ids=pc.case_id)
def test_abs_ldr_is_the_dense_operator(c):
    ref = pc.reference(c)
    o = ref["o"]
    D = o.dense(o.apply_op_Ldr)
    ax = np.abs(ref["states"][1]["x"])
    got, d = pc.abs_ldr(o, ax)
    want = (np.abs(D) @ ax.reshape(ax.shape[0], -1).T).T.reshape(ax.shape)
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)
    assert d == int((D != 0).sum(1).max())
    assert (got[:, 0] == 0).all() and (got[:, 1:] >= ax[:, 1:]).all()
