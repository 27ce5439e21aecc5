"""The feature-space novelty score on the host: the float64 definition of tests/_novelty.py against
the two-pass textbook form, its independence of the pivot, the finalising algebra, statistical
sanity, and cilrs_mi355.novelty.FeatureDensity with its launches replaced by the definition.

Bounds.  The moment form against the two-pass form: 1e-10 relative to max|Sigma| (both are float64
sums of N ~ 1e3 products: N 2^-53 ~ 1e-13, times the cancellation G - sum n mu mu^T the pivot keeps
near 1).  Pivot independence: the zero pivot loses mean^2 / variance (< 10 here) to that
cancellation and the triangular factor amplifies by at most cond(Sigma_l), which the shrinkage
bounds: lambda_max(Sigma) <= tr Sigma = F t and lambda_min(Sigma_l) >= l t, so
cond(Sigma_l) <= 1 + (1 - l) F / l = 1 + 99 F at l = 0.01 (6.4e3 at F = 64):
7e-14 * 10 * 6.4e3 < 1e-8 relative to max|W|.
"""
import numpy as np
import pytest
import torch

import _novelty as N
from cilrs_mi355.novelty import FeatureDensity, finalize_tables, table_doubles

F0, NC0, LAM = 64, 4, 0.01


def _fit(F=F0, NC=NC0, rows=600, seed=1, pivot="first", batch=50, dead=0.1):
    v, cmd = N.relu_features(rows, F, NC, seed, dead=dead)
    piv = v[:batch].mean(axis=0, dtype=np.float32) if pivot == "first" else np.zeros(F, np.float32)
    t = None
    for b0 in range(0, rows, batch):
        t = N.moments(v[b0:b0 + batch], cmd[b0:b0 + batch], piv, NC, t)
    return v, cmd, piv, t


def test_shifted_moments_equal_the_two_pass_definition():
    v, cmd, piv, t = _fit()
    fin = N.finalize(t, piv, F0, NC0, LAM)
    sigma, mean, present = N.two_pass(v, cmd, NC0)
    assert present.all() and fin["present"].all() and fin["N"] == 600 and fin["Kp"] == NC0
    rel = np.abs(fin["sigma"] - sigma).max() / np.abs(sigma).max()
    relm = np.abs(fin["mean"] - mean).max() / np.abs(mean).max()
    print(f"moments vs two-pass: Sigma {rel:.3g}, means {relm:.3g}")
    assert rel <= 1e-10 and relm <= 1e-10
    assert (np.diag(sigma) == 0.0).any(), "the synthetic features must have dead channels"


def test_result_does_not_depend_on_the_pivot():
    _v, _c, p1, t1 = _fit(pivot="first")
    _v, _c, p0, t0 = _fit(pivot="zero")
    a, b = N.finalize(t1, p1, F0, NC0, LAM), N.finalize(t0, p0, F0, NC0, LAM)
    rel = np.abs(a["W"] - b["W"]).max() / np.abs(a["W"]).max()
    relm = np.abs(a["mean"] - b["mean"]).max() / np.abs(a["mean"]).max()
    print(f"pivot first-batch mean vs zero: W {rel:.3g}, means {relm:.3g}")
    assert rel <= 1e-8 and relm <= 1e-12


def test_score_is_the_quadratic_form_of_the_shrunk_covariance():
    v, cmd, piv, t = _fit()
    fin = N.finalize(t, piv, F0, NC0, LAM)
    u = v[:40].astype(np.float64) - fin["mean"][cmd[:40]]
    y = u @ fin["W"].T
    want = np.einsum("bi,bi->b", u, np.linalg.solve(fin["sigma_l"], u.T).T)
    rel = np.abs((y * y).sum(axis=1) - want).max() / want.max()
    print(f"|W u|^2 vs u^T Sigma_l^-1 u: {rel:.3g}")
    assert rel <= 1e-9
    assert np.array_equal(fin["W"], np.tril(fin["W"]))


@pytest.mark.parametrize("F,rows", [(128, 60), (128, 700), (512, 200)])
def test_dead_channels_and_few_rows_finalise_under_the_default_shrinkage(F, rows):
    v, cmd, piv, t = _fit(F=F, rows=rows, batch=20, dead=0.2)
    fin = N.finalize(t, piv, F, NC0, LAM)
    assert np.isfinite(fin["W"]).all() and np.isfinite(fin["W32"]).all()
    cond = np.linalg.cond(fin["sigma_l"])
    print(f"F {F} N {rows}: cond(Sigma_l) {cond:.3g}, rank(Sigma) <= {min(rows - NC0, F)}")
    assert cond <= 1.0 + (1.0 - LAM) * F / LAM          # whatever the features: see the docstring
    d2, _ = N.score(v, cmd, fin["mean32"], fin["W32"])
    assert np.isfinite(d2).all() and (d2 > 0).all()


def test_a_command_with_no_sample_gets_no_mean():
    v, cmd = N.relu_features(300, F0, NC0, 5)
    cmd[cmd == 2] = 1
    piv = v[:50].mean(axis=0, dtype=np.float32)
    fin = N.finalize(N.moments(v, cmd, piv, NC0), piv, F0, NC0, LAM)
    assert fin["present"].tolist() == [True, True, False, True] and fin["Kp"] == 3
    assert not fin["mean"][2].any()
    sigma, _m, _p = N.two_pass(v, cmd, NC0)
    assert np.abs(fin["sigma"] - sigma).max() / np.abs(sigma).max() <= 1e-10
    # an out-of-range command counts as command 0
    cmd2 = cmd.copy()
    cmd2[cmd2 == 0] = 9
    fin2 = N.finalize(N.moments(v, cmd2, piv, NC0), piv, F0, NC0, LAM)
    assert np.array_equal(fin2["W"], fin["W"]) and np.array_equal(fin2["mean"], fin["mean"])


def test_statistical_sanity_of_gaussian_rows():
    F, NC, n_fit, M = 16, 3, 20000, 2000
    rng = np.random.default_rng(7)
    A = rng.standard_normal((F, F)) / np.sqrt(F) + np.eye(F)
    mu = rng.standard_normal((NC, F))

    def draw(n):
        k = rng.integers(0, NC, size=n)
        return (mu[k] + rng.standard_normal((n, F)) @ A.T).astype(np.float32), k

    v, k = draw(n_fit)
    piv = v[:128].mean(axis=0, dtype=np.float32)
    fin = N.finalize(N.moments(v, k, piv, NC), piv, F, NC, 0.0)
    fresh, kf = draw(M)
    tol = 5.0 * np.sqrt(2.0 * F / M)
    d2, _ = N.score(fresh, kf, fin["mean32"], fin["W32"])
    shifted = (fresh.astype(np.float64) + 3.0 * fin["L"][:, 0][None, :]).astype(np.float32)
    d2s, _ = N.score(shifted, kf, fin["mean32"], fin["W32"])
    print(f"in-distribution mean d2 {d2.mean():.2f} (F = {F}), shifted {d2s.mean():.2f} (F + 9 = "
          f"{F + 9}), tolerance {tol:.2f}")
    assert abs(d2.mean() - F) <= tol
    assert abs(d2s.mean() - (F + 9)) <= tol


# ---- FeatureDensity with the launches replaced by the definition ----------------------------------
class _Stub:
    """what FeatureDensity reads of a model"""
    training = False

    def __init__(self, F=F0, NC=NC0):
        self.FEATURES, self.num_commands = F, NC
        self._p = torch.zeros(1)

    def parameters(self):
        return iter([self._p])


class _HostDensity(FeatureDensity):
    def _moments_op(self, features, commands):
        t = N.moments(features[:, :self.F].numpy(), commands.numpy(), self.pivot.numpy(), self.NC,
                      self.table.numpy())
        self.table.copy_(torch.from_numpy(t))
        if ((commands < 0) | (commands >= self.NC)).any():
            self.status.fill_(1)

    def _score_op(self, features, commands, d2):
        got, _ = N.score(features.numpy(), commands.numpy(), self.mean.numpy(), self.W.numpy())
        d2.copy_(torch.from_numpy(got.astype(np.float32)))


def _fitted(rows=400, seed=3):
    v, cmd = N.relu_features(rows + 100, F0, NC0, seed)
    v = np.concatenate([v, np.full((len(v), 8), np.nan, np.float32)], axis=1)      # ld = F + 8
    vt, ct = torch.from_numpy(v), torch.from_numpy(cmd)
    fd = _HostDensity(_Stub(), capacity=16)
    for b0 in range(0, rows, 50):
        fd.update_features(vt[b0:b0 + 50], ct[b0:b0 + 50])
    return fd, vt, ct, rows


def test_feature_density_round_trip(tmp_path):
    fd, vt, ct, rows = _fitted()
    assert not fd.finalized
    assert fd.finalize() is fd and fd.finalized and fd.count == rows
    v, cmd = vt[:rows, :F0].numpy(), ct[:rows].numpy()
    fin = N.finalize(N.moments(v, cmd, fd.pivot.numpy(), NC0), fd.pivot.numpy(), F0, NC0, LAM)
    # the pivot is the first batch's column mean (any rounding of it will do: the fit does not
    # depend on it)
    assert np.abs(fd.pivot.numpy() - v[:50].mean(axis=0, dtype=np.float64)).max() <= 1e-6
    relw = np.abs(fd.W.numpy() - fin["W32"]).max() / np.abs(fin["W32"]).max()
    assert relw <= 1e-6 and np.abs(fd.mean.numpy() - fin["mean32"]).max() <= 1e-6
    m64, W64, present, n = finalize_tables(fd.table.numpy(), fd.pivot.numpy(), F0, NC0, LAM)
    assert np.abs(W64 - fin["W"]).max() / np.abs(fin["W"]).max() <= 1e-12
    assert np.abs(m64 - fin["mean"]).max() <= 1e-12 and present.all() and n == rows
    assert fd.table.numel() == table_doubles(F0, NC0) == N.table_doubles(F0, NC0)
    for b0 in range(rows, rows + 100, 30):                   # the log grows past its capacity
        fd.calibrate_features(vt[b0:b0 + 30], ct[b0:b0 + 30])
    assert fd.log_count == 100
    s = fd.calibration_scores()
    assert s.shape == (100,) and np.all(np.diff(s) >= 0)
    qs = [fd.quantile(q) for q in (0.0, 0.5, 0.9, 1.0)]
    assert qs == sorted(qs) and qs[0] == s[0] and qs[-1] == s[-1]
    grid = np.linspace(0.0, float(s[-1]) * 1.5, 64, dtype=np.float32)
    pc = fd.percentile(grid)
    assert np.all(np.diff(pc) >= 0) and pc[0] == 0.0 and pc[-1] == 100.0
    assert fd.percentile(float(s[49])) == 50.0 == fd.percentile(np.float32(s[49]))
    d2 = fd.score_features(vt[:7], ct[:7])
    path = tmp_path / "density.pth"
    fd.save(path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert set(sd) == {"F", "NC", "shrinkage", "count", "weights_key", "finalized", "table", "pivot",
                       "mean", "W", "present", "calibration"}
    fd2 = _HostDensity(_Stub(), shrinkage=0.5)
    assert fd2.load(path) is fd2
    assert fd2.finalized and fd2.shrinkage == LAM and fd2.count == rows
    for a, b in ((fd.table, fd2.table), (fd.pivot, fd2.pivot), (fd.mean, fd2.mean), (fd.W, fd2.W)):
        assert torch.equal(a, b)
    assert np.array_equal(fd2.calibration_scores(), s) and np.array_equal(fd2.present, fd.present)
    assert torch.equal(fd2.score_features(vt[:7], ct[:7]), d2)
    assert fd2.percentile(float(s[10])) == fd.percentile(float(s[10]))
    # a density saved before finalize() resumes its fit
    fd3, vt3, ct3, _ = _fitted(rows=100)
    fd4 = _HostDensity(_Stub()).load_state_dict(fd3.state_dict())
    assert not fd4.finalized and torch.equal(fd4.table, fd3.table)
    fd3.update_features(vt3[100:150], ct3[100:150])
    fd4.update_features(vt3[100:150], ct3[100:150])
    assert torch.equal(fd3.finalize().W, fd4.finalize().W)


def test_feature_density_errors():
    fd, vt, ct, rows = _fitted(rows=100)
    for call in (lambda: fd.score_features(vt[:2], ct[:2]), lambda: fd.quantile(0.5),
                 lambda: fd.percentile(1.0), lambda: fd.calibrate([]),
                 lambda: fd.check_commands([0]), lambda: fd.calibrate_features(vt[:2], ct[:2])):
        with pytest.raises(RuntimeError, match="finalize"):
            call()
    with pytest.raises(RuntimeError, match="no rows"):
        _HostDensity(_Stub()).finalize()
    fd.finalize()
    with pytest.raises(RuntimeError, match="already finalised"):
        fd.update_features(vt[:2], ct[:2])
    with pytest.raises(RuntimeError, match="no calibration"):
        fd.quantile(0.5)
    with pytest.raises(RuntimeError, match="features"):
        fd.check_model(_Stub(F=2 * F0))
    with pytest.raises(RuntimeError, match="commands"):
        fd.check_model(_Stub(NC=NC0 + 2))
    fd.check_model(_Stub())
    with pytest.raises(RuntimeError, match="features"):
        _HostDensity(_Stub(F=2 * F0)).load_state_dict(fd.state_dict())
    with pytest.raises(RuntimeError, match="commands"):
        _HostDensity(_Stub(NC=2)).load_state_dict(fd.state_dict())
    with pytest.raises(RuntimeError, match="float32"):
        fd.score_features(vt[:2, :F0 - 1], ct[:2])
    with pytest.raises(RuntimeError, match="out of range"):
        fd.check_commands([NC0])
    for lam in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            _HostDensity(_Stub(), shrinkage=lam)
    # a command the fit never saw has no mean: scoring it raises
    v, cmd = N.relu_features(200, F0, NC0, 9)
    cmd[cmd == 3] = 0
    gap = _HostDensity(_Stub())
    gap.update_features(torch.from_numpy(v), torch.from_numpy(cmd))
    gap.finalize()
    assert gap.present.tolist() == [True, True, True, False]
    with pytest.raises(RuntimeError, match="never occurred"):
        gap.score_features(torch.from_numpy(v[:2]), torch.tensor([0, 3]))
    gap.score_features(torch.from_numpy(v[:2]), torch.tensor([0, 2]))
    # an out-of-range command during the fit raises at finalize()
    bad = _HostDensity(_Stub())
    cmd[0] = 7
    bad.update_features(torch.from_numpy(v), torch.from_numpy(cmd))
    with pytest.raises(RuntimeError, match="out of range"):
        bad.finalize()
    # without a device there is no fallback
    plain = FeatureDensity(_Stub())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        plain.update_features(torch.from_numpy(v), torch.from_numpy(cmd))
