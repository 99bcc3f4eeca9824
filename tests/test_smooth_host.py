"""CPU: the reference of the spatial smoothness prior (tests/smooth_ref.py) is self-consistent --
its gradient against central finite differences, quad against huber, the host neighbour table's
invariants -- and solve()'s validation of the smoothness arguments, which needs no device."""
import numpy as np
import pytest
import torch

import smooth_ref as sr


def _field(seed, R, I, J, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.rand(R, 1, I, J, generator=g, dtype=torch.float64)).numpy()


@pytest.mark.parametrize("kind,delta", [("quad", None), ("huber", 0.2)])
@pytest.mark.parametrize("shape", [(2, 5, 7), (3, 1, 9), (1, 6, 1)])
def test_ref_gradient_matches_finite_differences(kind, delta, shape):
    R, I, J = shape
    S = _field(5, R, I, J)
    if kind == "huber":  # both branches occur (differences of U(0,1) values against delta = 0.2)
        d = np.abs(np.diff(S.reshape(R, I, J), axis=2 if J > 1 else 1))
        assert (d < delta).any() and (d > delta).any()
    v, g = sr.penalty(S, kind, delta)
    h = 1e-6
    fd = np.zeros_like(S)
    for idx in np.ndindex(*S.shape):
        Sp, Sm = S.copy(), S.copy()
        Sp[idx] += h
        Sm[idx] -= h
        fd[idx] = (sr.penalty(Sp, kind, delta)[0] - sr.penalty(Sm, kind, delta)[0]) / (2 * h)
    # central differences of a piecewise quadratic: exact up to rounding, v * eps / h ~ 1e-9
    assert np.allclose(g, fd, rtol=0, atol=1e-7)
    assert v > 0


def test_quad_equals_delta_times_huber_inside_the_quadratic_zone():
    S = _field(6, 3, 8, 5)
    delta = 2.0  # exceeds every difference of values in [0, 1]
    vq, gq = sr.penalty(S, "quad")
    vh, gh = sr.penalty(S, "huber", delta)
    assert np.isclose(vq, delta * vh, rtol=1e-13)
    assert np.allclose(gq, delta * gh, rtol=1e-13, atol=0)


def test_ref_gradient_closed_form():
    """quad: sum over neighbours of (S(p) - S(n)); huber: the clamped differences."""
    R, I, J = 2, 4, 6
    S = _field(7, R, I, J)
    X = S.reshape(R, I, J)
    for kind, delta in (("quad", None), ("huber", 0.3)):
        g = np.zeros_like(X)
        for i in range(I):
            for j in range(J):
                for di, dj in ((0, -1), (0, 1), (-1, 0), (1, 0)):
                    a, c = i + di, j + dj
                    if 0 <= a < I and 0 <= c < J:
                        d = X[:, i, j] - X[:, a, c]
                        g[:, i, j] += d if kind == "quad" else np.clip(d / delta, -1, 1)
        assert np.allclose(sr.penalty(S, kind, delta)[1].reshape(R, I, J), g, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("I,J,pads", [(5, 7, 29), (1, 9, 3), (6, 1, 0)])
def test_host_neighbour_table_invariants(I, J, pads):
    P = I * J
    rng = np.random.default_rng(3)
    perm = np.concatenate([rng.permutation(P), np.full(pads, -1)]).astype(np.int32)
    rng.shuffle(perm)  # pads anywhere
    nbr = sr.neighbor_table(perm, I, J)
    Pp = P + pads
    assert nbr.shape == (Pp, 4) and nbr.dtype == np.int32
    for q in range(Pp):
        p = perm[q]
        if p < 0:
            assert (nbr[q] == -1).all()  # pads
            continue
        i, j = divmod(int(p), J)
        # the border gives -1, the interior a position
        assert (nbr[q, 0] == -1) == (j == 0)
        assert (nbr[q, 1] == -1) == (j == J - 1)
        assert (nbr[q, 2] == -1) == (i == 0)
        assert (nbr[q, 3] == -1) == (i == I - 1)
        for slot, back, dp in ((0, 1, -1), (1, 0, 1), (2, 3, -J), (3, 2, J)):
            n = nbr[q, slot]
            if n >= 0:
                assert perm[n] == p + dp
                assert nbr[n, back] == q  # symmetry: left of q' <=> right of q
    # ... and in the other direction: whoever names q as its right neighbour is q's left one
    for q in range(Pp):
        for slot, back in ((0, 1), (1, 0), (2, 3), (3, 2)):
            for n in np.nonzero(nbr[:, slot] == q)[0]:
                assert nbr[q, back] == n


def test_solve_validates_the_smoothness_arguments():
    """Raised before anything touches a device."""
    from quantized_spectrum_cartography_amd import qmc
    Y = torch.zeros(4, 1, 6, 6, dtype=torch.int64)
    Wx = torch.ones(4, 1, 6, 6)
    b = torch.tensor([0.0, 0.5, 1.0])
    kw = dict(R=2, max_iter=1)
    with pytest.raises(ValueError, match="smooth must be >= 0"):
        qmc.solve(Y, Wx, b, 0.1, smooth=-1.0, **kw)
    with pytest.raises(ValueError, match="smooth_kind"):
        qmc.solve(Y, Wx, b, 0.1, smooth=1.0, smooth_kind="tv", **kw)
    with pytest.raises(ValueError, match="smooth_delta"):
        qmc.solve(Y, Wx, b, 0.1, smooth=1.0, smooth_kind="huber", **kw)
    with pytest.raises(ValueError, match="smooth_delta"):
        qmc.solve(Y, Wx, b, 0.1, smooth=1.0, smooth_kind="huber", smooth_delta=0.0, **kw)
    with pytest.raises(ValueError, match="generator"):
        qmc.solve(Y, Wx, b, 0.1, smooth=1.0, generator=torch.nn.Identity(),
                  Z_init=torch.zeros(2, 36), **kw)


def test_fp32_restatement_of_the_solver_reference_runs():
    """free_s_solve_smooth in fp32 (the oracle's own functions) and fp64 agree on a tiny case: the
    two data terms are the same expression."""
    from oracle import reference_ops as ro
    g = torch.Generator().manual_seed(11)
    R, I, J, K = 2, 6, 5, 4
    S = torch.rand(R, 1, I, J, generator=g)
    C = torch.rand(R, K, generator=g)
    Tt = ro.get_tensor(S, C)
    b = torch.tensor([0.0, float(Tt.median()), float(Tt.max()) + 1.0])
    Y = ro.quantize(Tt, 0.2, b, noise=torch.randn(Tt.shape, generator=g)).unsqueeze(1)
    Wx = torch.bernoulli(torch.full((K, 1, I, J), 0.5), generator=g)
    S0 = 0.1 + 0.5 * torch.rand(R, 1, I, J, generator=g)
    C0 = 0.1 + 0.5 * torch.rand(R, K, generator=g)
    kw = dict(n_iter=3, smooth=2.0, kind="huber", delta=0.1)
    a = sr.free_s_solve_smooth(S0, C0, Y, Wx, b, 0.2, dtype=torch.float64, **kw)
    c = sr.free_s_solve_smooth(S0, C0, Y, Wx, b, 0.2, dtype=torch.float32, **kw)
    assert np.allclose(c["S"].double().numpy(), a["S"].numpy(), rtol=0, atol=1e-5)
    assert np.allclose(c["costs_s"], a["costs_s"], rtol=1e-5)
    # the prior is in the cost: without it the recorded cost is lower by smooth * R(S0)
    z = sr.free_s_solve_smooth(S0, C0, Y, Wx, b, 0.2, n_iter=1)
    pen0 = sr.penalty(S0.double().numpy(), "huber", 0.1)[0]
    assert np.isclose(a["costs_c"][0] - z["costs_c"][0], 2.0 * pen0, rtol=1e-9)
