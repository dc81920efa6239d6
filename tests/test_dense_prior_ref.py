"""The declared semantics of the dense keyframe prior and of the marginalisation that produces one (tests/dense_prior_ref.py), checked
against themselves on the CPU: the tangent Jacobian against central differences in long double, the long-double Schur complement against
a brute-force minimisation of the same model, positive semi-definiteness of what a Huber-active problem leaves, and the C-ABI surface."""
import ctypes

import numpy as np

from tests import dense_prior_ref as dp

LD = dp.LD


def _state(rng, n_sel):
    x0 = np.zeros((n_sel, 16))
    x0[:, :4] = rng.normal(size=(n_sel, 4)) * rng.uniform(0.7, 1.4, (n_sel, 1))      # un-normalised: the normalisation is part of the code
    x0[:, 4:] = rng.normal(size=(n_sel, 12))
    return x0


def _moved(rng, x0, angles):
    eps = rng.normal(size=15 * len(x0)) * 0.3
    for k, a in enumerate(angles):
        d = rng.normal(size=3)
        eps[15 * k:15 * k + 3] = a * d / np.linalg.norm(d)
    x = dp.state_plus(x0, eps)
    x[:, :4] *= rng.uniform(0.6, 1.5, (len(x0), 1))
    return x


def test_tangent_jacobian_against_central_differences_in_long_double():
    """T, the gradient and the Gauss-Newton matrix at 1e-3, 0.5, pi/2 - 1e-3 (d.w close to 0) and 2.2 rad (d.w < 0) from x0.  Central
    differences with h = 1e-6 in long double: truncation ~ h^2, rounding ~ 1e-19 / h, so 1e-10 bounds both with two digits to spare."""
    rng = np.random.default_rng(4)
    angles = [1e-3, 0.5, np.pi / 2 - 1e-3, 2.2]
    x0 = _state(rng, 4)
    x = _moved(rng, x0, angles)
    e = dp.local(x, x0)
    for k, a in enumerate(angles):
        want = a if a < np.pi / 2 else np.pi - a
        assert abs(np.linalg.norm(e[15 * k:15 * k + 3]) - want) <= 1e-12
    T = dp.tangent_jacobian(x, x0)
    h = LD(1e-6)
    xl, x0l = x.astype(LD), x0.astype(LD)
    J = np.zeros((60, 60), LD)
    for j in range(60):
        d = np.zeros(60, LD); d[j] = h
        J[:, j] = (dp.local(dp.state_plus(xl, d), x0l) - dp.local(dp.state_plus(xl, -d), x0l)) / (2 * h)
    assert float(np.abs(J - T).max()) <= 1e-10
    A = rng.normal(size=(70, 60))
    info, eta, c0 = A.T @ A, rng.normal(size=60), 3.0
    cost, g, H = dp.evaluate(x0, info, eta, c0, x)
    gd = np.zeros(60, LD)
    for j in range(60):
        d = np.zeros(60, LD); d[j] = h
        cp = dp.evaluate(x0l, info.astype(LD), eta.astype(LD), LD(c0), dp.state_plus(xl, d))[0]
        cm = dp.evaluate(x0l, info.astype(LD), eta.astype(LD), LD(c0), dp.state_plus(xl, -d))[0]
        gd[j] = (cp - cm) / (2 * h)
    assert float(np.abs(gd - g).max()) <= 1e-10 * max(1.0, float(np.abs(g).max()))
    assert np.abs(H - T.T @ dp.sym_lower(info) @ T).max() <= 1e-12 * np.abs(H).max()
    # Plus(x0, e) = x up to the quaternion's norm and sign
    back = dp.state_plus(x0, e)
    for k in range(4):
        u, v = back[k, :4] / np.linalg.norm(back[k, :4]), x[k, :4] / np.linalg.norm(x[k, :4])
        assert min(np.abs(u - v).max(), np.abs(u + v).max()) <= 1e-12
    assert np.abs(back[:, 4:] - x[:, 4:]).max() <= 1e-12


def test_tangent_jacobian_is_the_identity_at_x0():
    rng = np.random.default_rng(5)
    x0 = _state(rng, 3)
    # (u (x) u0^-1 is the identity up to the rounding of its four-term sums: |delta| <= 4 * 2^-53, and T - I = -[delta]x + O(delta^2))
    assert np.abs(dp.tangent_jacobian(x0, x0) - np.eye(45)).max() <= 8 * 2.0 ** -53 and np.abs(dp.local(x0, x0)).max() <= 8 * 2.0 ** -53
    x = x0.copy(); x[:, :4] *= -2.5                  # the same rotations: another norm, the other sign
    assert np.abs(dp.tangent_jacobian(x, x0) - np.eye(45)).max() <= 1e-15 and np.abs(dp.local(x, x0)).max() <= 1e-15
    A = rng.normal(size=(50, 45))
    info, eta = A.T @ A, rng.normal(size=45)
    cost, g, H = dp.evaluate(x0, info, eta, 0.25, x0)
    big = np.abs(info).max()
    assert abs(cost - 0.25) <= 1e-13 and np.abs(g - eta).max() <= 1e-13 * big and np.abs(H - dp.sym_lower(info)).max() <= 1e-13 * big
    # only the lower triangle is read; a constant block has zero columns
    junk = info + np.triu(rng.normal(size=info.shape), 1)
    assert np.array_equal(dp.evaluate(x0, junk, eta, 0.25, x0)[2], H)
    _, gc, Hc = dp.evaluate(x0, info, eta, 0.25, x0, const_bits=[1, 4, 0])
    off = np.r_[0:6, 24:27]
    assert not gc[off].any() and not Hc[off, :].any() and not Hc[:, off].any()
    on = np.setdiff1d(np.arange(45), off)
    assert np.abs(Hc[np.ix_(on, on)] - H[np.ix_(on, on)]).max() <= 1e-13 * big


def _huber_problem(rng, d, n_blocks, a):
    """random linearised blocks of two residuals each with Ceres' Huber corrector (rho'' <= 0 branch): H, g of the robustified rows and the
    cost 1/2 sum rho, half the blocks beyond the threshold"""
    J = rng.normal(size=(2 * n_blocks, d))
    r = rng.normal(size=2 * n_blocks) * np.repeat(np.where(np.arange(n_blocks) % 2 == 0, 0.2 * a, 3.0 * a), 2)
    cost, active = 0.0, 0
    for b in range(n_blocks):
        s = r[2 * b] ** 2 + r[2 * b + 1] ** 2
        if s > a * a:
            rho, sc = 2 * a * np.sqrt(s) - a * a, np.sqrt(a / np.sqrt(s))
            active += 1
        else:
            rho, sc = s, 1.0
        cost += 0.5 * rho
        J[2 * b:2 * b + 2] *= sc; r[2 * b:2 * b + 2] *= sc
    return J.T @ J, J.T @ r, cost, active, 0.5 * float(r @ r)


def test_marginal_prior_against_brute_force_minimisation():
    rng = np.random.default_rng(6)
    H, g, c, _, _ = _huber_problem(rng, 45, 60, 1.0)
    H[7, :] = 0; H[:, 7] = 0; g[7] = 0                # an absent unknown in the rest
    H[31, :] = 0; H[:, 31] = 0; g[31] = 0             # and one in the selection
    sel = dp.natural_index(3, [1, 0])                 # 30 of the 45, unordered
    info, eta, c0 = dp.marginal_prior(H, g, c, sel)
    bi, be, bc = dp.brute_force(H, g, c, sel)
    scale = float(np.abs(info).max())
    assert float(np.abs(info - bi).max()) <= 1e-15 * scale and float(np.abs(eta - be).max()) <= 1e-15 * scale and abs(float(c0 - bc)) <= 1e-15 * scale
    where = list(sel).index(31)
    assert not info[where].any() and not info[:, where].any() and eta[where] == 0
    # everything selected: the model itself
    i2, e2, c2 = dp.marginal_prior(H, g, c, np.arange(45))
    assert np.array_equal(i2.astype(np.float64), dp.sym_lower(H)) and np.array_equal(e2.astype(np.float64), g) and float(c2) == c
    # the float64 computation stays within its own bound of the reference
    A = dp.augmented(info, eta, c0)
    assert dp.err64_bound(H, g, c, sel, A, 3) <= 1e-12


def test_huber_active_problem_leaves_a_positive_semidefinite_prior():
    rng = np.random.default_rng(7)
    H, g, c, active, half_rr = _huber_problem(rng, 45, 80, 0.7)
    assert active >= 30 and c > half_rr * 1.05, "the corrector must be active: rho > rho' s"
    sel = dp.natural_index(3, [2])
    info, eta, c0 = dp.marginal_prior(H, g, c, sel)
    A = dp.augmented(info, eta, c0).astype(np.float64)
    w = np.linalg.eigvalsh(A)
    assert w.min() >= -1e-12 * w.max() and float(c0) >= 0.0
    # with the quadratic loss' constant 1/2 |r~|^2 in place of 1/2 sum rho the corner is smaller by exactly the difference
    c0_q = dp.marginal_prior(H, g, half_rr, sel)[2]
    assert abs(float(c0 - c0_q) - (c - half_rr)) <= 1e-12 * c
    # least-squares rows of the prior reproduce it
    Arows, b, const = dp.sqrt_rows(info.astype(np.float64), eta.astype(np.float64), float(c0))
    e = rng.normal(size=15)
    want = float(c0) + float(eta.astype(np.float64) @ e) + 0.5 * float(e @ info.astype(np.float64) @ e)
    assert abs(0.5 * float((Arows @ e + b) @ (Arows @ e + b)) + const - want) <= 1e-10 * abs(want)


def test_new_symbols_are_declared_and_exported():
    from lvio_fusion_amd import _lib, api
    declared = _lib.declared_symbols()
    so = ctypes.CDLL(_lib.SO_PATH)
    for n in ("lvf_dense_prior_create", "lvf_dense_prior_destroy", "lvf_dense_prior_size", "lvf_dense_prior_download", "lvf_dense_prior_evaluate",
              "lvf_problem_set_dense_prior", "lvf_problem_marginal_prior", "lvf_window_set_dense_prior", "lvf_window_get_dense_prior",
              "lvf_window_slide_marginalize"):
        assert n in declared and n in _lib._SIGS, n
        getattr(so, n)
    for cls, names in ((api.Problem, ("set_dense_prior", "marginal_prior")), (api.Window, ("set_dense_prior", "get_dense_prior", "slide_marginalize"))):
        for n in names:
            assert callable(getattr(cls, n)), n
    assert callable(api.DensePrior)
