"""The float64 restatement (oracle/admm_oracle.py) with time-varying edge weights: ``u_ew`` of shape (T, N, k), ``d_ew`` of shape
(T-1, N, k+1), one CSR matrix per time slice.

The reference multiplies its tables slice by slice (ADMM.py:147, 171, 200, 214):
  Lu    at time t reads slice t of u_ew;
  Ldr   at time t >= 1 reads slice t-1 of d_ew (the edges from step t-1 to t);
  Ldr_T at time t <= T-2 reads slice t of d_ew, transposed in kNN mode (scatter_add), as it stands in physical mode (gather).
Everything above the three operators -- left-hand sides, CG, the ADMM loop, the histories -- is inherited unchanged.
tests/test_tv_oracle_golden.py pins this class against tests/golden/g11_time_varying.npz, the reference's own output."""
import numpy as np

from oracle import admm_oracle as orc


class TvOracleADMM(orc.OracleADMM):
    def __init__(self, cl, u_ew, d_ew, ADMM_info, *, mode="knn", **kw):
        assert mode in ("knn", "physical")
        u_ew, d_ew = np.asarray(u_ew, dtype=np.float32), np.asarray(d_ew, dtype=np.float32)
        super().__init__(cl, u_ew[0], d_ew[0], ADMM_info, mode=mode, **kw)
        assert u_ew.shape[0] == self.T and d_ew.shape[0] == self.T - 1, (u_ew.shape, d_ew.shape, self.T)
        self.Wu_t = [orc.tables_to_csr(self.cl, w, None)[0] for w in u_ew]
        self.Wd_t = [orc.tables_to_csr(self.cl, u_ew[0], w)[1] for w in d_ew]
        self.WdT_t = [W.T.tocsr() if mode == "knn" else W for W in self.Wd_t]
        self.Wu = self.Wd = self.WdT = None      # nothing inherited may read one slice for all

    def _sp_t(self, Ws, x):
        """y[:, j] = Ws[j] x[:, j] for the len(Ws) time slices of x."""
        assert x.shape[1] == len(Ws)
        return np.concatenate([self._sp(W, x[:, j:j + 1]) for j, W in enumerate(Ws)], axis=1)

    def apply_op_Lu(self, x):
        return x - self._sp_t(self.Wu_t[:x.shape[1]], x)

    def apply_op_Ldr(self, x):
        y = np.zeros_like(x)
        y[:, 1:] = x[:, 1:] - self._sp_t(self.Wd_t[:x.shape[1] - 1], x[:, :-1])
        return y

    def apply_op_Ldr_T(self, x):
        y = x.copy()
        ff = self._sp_t(self.WdT_t[:x.shape[1] - 1], x[:, 1:])
        y[:, :-1] = x[:, :-1] - ff
        if not self.bug_compat:
            y[:, 0] = -ff[:, 0]
        return y

    def apply_op_Ln(self, x):
        raise NotImplementedError("apply_op_Ln on time-varying tables is not restated")
