"""GPU: the logistic (ordered-logit) observation model, loss="logit", through the elementwise ops,
the fused passes and the solvers, against the goldens of tools/make_golden_logit.py and the CPU
restatement of tests/logit_ref.py.

Tolerances are the project's own for the same comparisons (tests/test_gpu_fused.py): 1e-5
relative (Frobenius) for passes and solves, rtol 1e-5 for cost histories."""
import numpy as np
import pytest
import torch

import logit_ref as lr
from conftest import rel_fro
from test_gpu_fused import _random_case

pytestmark = pytest.mark.gpu

T = torch.from_numpy


def _obs(Y, Wx, b, s, offset=0.0, log_model=False, R=4, tile=None, **kw):
    from quantized_spectrum_cartography_amd.obs import Observations
    return Observations(Y, Wx, b, s, offset=offset, log_model=log_model, R_hint=R, tile=tile,
                        loss="logit", **kw)


def _gin(g):
    return dict(S0=T(g["S0"]), C0=T(g["C0"]), Y=T(g["Y"].astype(np.int64)),
                Wx=T(g["Wx"].astype(np.float32)), b=T(g["b"]), s=float(g["sigma"]),
                offset=float(g["offset"]), log_model=bool(g["log_model"]))


# ---------------------------------------------------------------------------------------
# elementwise ops
# ---------------------------------------------------------------------------------------
def test_f_logit_matches_reference():
    from quantized_spectrum_cartography_amd import quantization_model as qm
    # |y / s| <= 16: the fp32 rounding of y / s alone moves exp(-|y / s|) by 16 * 2^-24 = 1e-6
    # relative; a few ulp of exp, the reciprocal and the product on top -> 3e-6
    y = torch.linspace(-8, 8, 1001)
    for s in (1.0, 0.5):
        out = qm.F_logit(y.cuda(), s).cpu()
        ref = 1.0 / (1.0 + torch.exp(-y.double() / s))
        assert torch.allclose(out.double(), ref, rtol=3e-6, atol=0)
        # the reference form loses relative precision only near F = 1 (absolute 2^-24)
        assert torch.allclose(out, lr.F_logit(y, s), rtol=3e-6, atol=1.2e-7)
    # both tails stay finite and monotone where 1/(1+exp(-y)) overflows
    far = qm.F_logit(torch.tensor([-200.0, 200.0]).cuda(), 1.0).cpu()
    assert far[0].item() == 0.0 and far[1].item() == 1.0


@pytest.mark.parametrize("name", ["pass_logit_small", "solve_logit_32"])  # linear, log model
def test_prob_logit_and_backward(golden, name):
    from quantized_spectrum_cartography_amd import _model
    d = _gin(golden(name))
    Th = lr.ro.get_tensor(d["S0"], d["C0"]).unsqueeze(1)
    X = torch.log(Th + d["offset"]) if d["log_model"] else Th
    Xg = X.clone().cuda().requires_grad_(True)
    P = _model.prob_logit(d["Y"].cuda(), Xg, d["b"], d["s"], log_model=d["log_model"])
    w = torch.linspace(0.5, 1.5, X.numel()).reshape(X.shape)
    (P * w.cuda()).sum().backward()
    # the reference formulation (fp32) and fp64 torch autograd of the plain expression
    Pr = lr.prob_logit(d["Y"], X, d["b"], d["s"], d["log_model"])
    assert torch.allclose(P.detach().cpu(), Pr, rtol=1e-5, atol=1e-7)
    e = torch.tensor(lr.explicit.edges_of(d["b"].numpy(), d["log_model"]))
    X64 = X.double().requires_grad_(True)
    P64 = torch.sigmoid((e[d["Y"] + 1] - X64) / d["s"]) - torch.sigmoid((e[d["Y"]] - X64) / d["s"])
    (P64 * w.double()).sum().backward()
    assert rel_fro(P.detach().cpu().numpy(), P64.detach().numpy()) < 1e-6
    assert rel_fro(Xg.grad.cpu().numpy(), X64.grad.numpy()) < 1e-5


def test_quantize_logit_bins_the_supplied_noise():
    from quantized_spectrum_cartography_amd import quantization_model as qm
    gen = torch.Generator().manual_seed(3)
    X = torch.rand(6, 10, 12, generator=gen)
    b = torch.tensor([0.0, 0.3, 0.6, 1.0])
    u = torch.rand(X.shape, generator=gen)
    L = torch.log(u) - torch.log1p(-u)
    Y = qm.quantize_logit(X.cuda(), 0.1, b, noise=L).cpu()
    ref = lr.ro.quantize(X, 0.1, b, noise=L)  # the same binning loop on x = X + noise * s
    assert torch.equal(Y, ref)
    torch.manual_seed(5)
    Y2 = qm.quantize_logit(X, 0.1, b)
    torch.manual_seed(5)
    u = torch.rand(X.shape)
    assert torch.equal(Y2, lr.ro.quantize(X, 0.1, b, noise=torch.log(u) - torch.log1p(-u)))


# ---------------------------------------------------------------------------------------
# fused pass
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pass_logit_small", "solve_logit_32"])
def test_logit_nll_pass_vs_golden(golden, name):
    from quantized_spectrum_cartography_amd import fused
    g = golden(name)
    d = _gin(g)
    R = d["S0"].shape[0]
    obs = _obs(d["Y"], d["Wx"], d["b"], d["s"], d["offset"], d["log_model"], R)
    S = d["S0"].cuda().requires_grad_(True)
    C = d["C0"].cuda().requires_grad_(True)
    nll = fused.ProbitNLL.apply(S, C, obs)
    cost = nll + float(g["lam_c"]) * torch.norm(C) + float(g["lam_s"]) * torch.norm(S)
    cost.backward()
    assert abs(nll.item() - float(g["nll"])) / abs(float(g["nll"])) < 1e-5
    assert abs(cost.item() - float(g["cost"])) / abs(float(g["cost"])) < 1e-5
    assert rel_fro(S.grad.cpu().numpy(), g["dS"]) < 1e-5
    assert rel_fro(C.grad.cpu().numpy(), g["dC"]) < 1e-5


_CASES = [
    (1, 1, 13, 11, 3, 0.5, 2, False, None),       # a: ragged, tiny
    (2, 3, 40, 40, 70, 0.1, 2, False, None),      # b: two k-slices
    (3, 8, 64, 64, 256, 0.1, 2, False, 512),      # c: the scpass path at RP 8
    (4, 16, 48, 50, 33, 0.2, 2, False, 192),      # d: rank 16
    (5, 4, 32, 32, 16, 0.3, 5, False, None),      # e: multi-bin
    (6, 4, 32, 32, 16, 0.3, 4, True, None),       # f: log model
    (7, 2, 51, 51, 64, 1.0, 2, False, None),      # g: every entry observed
]
_REFS = {}


def _explicit_ref(case):
    """The fp64 reference of a case, computed once and shared by its entry formats."""
    if case not in _REFS:
        seed, R, I, J, K, f, nbins, log_model, tile = case
        d = _random_case(seed, R, I, J, K, f, nbins, log_model)
        P = I * J
        ref = lr.nll_grad(d["S0"].reshape(R, P).numpy(), d["C0"].numpy(),
                          d["Y"].reshape(K, P).numpy(), d["Wx"].reshape(K, P).numpy(),
                          d["b"].numpy(), d["sigma"], d["offset"], log_model)
        _REFS[case] = (d, ref)
    return _REFS[case]


def _onebit(case):
    return case[6] == 2 and not case[7]


# one-bit cases once per entry format (1: signed rows, 0: code field); the others have one
_CASE_FMTS = [pytest.param(c, f, id="%s-fmt%d" % (n, f)) for c, n in zip(_CASES, "abcdefg")
              for f in ((1, 0) if _onebit(c) else (0,))]


@pytest.mark.parametrize("case,fmt", _CASE_FMTS)
def test_logit_pass_vs_explicit(case, fmt):
    """Fused pass against the explicit fp64 reference; one-bit cases once per entry format
    (signed rows, and code-field entries through Observations._fill(0))."""
    from quantized_spectrum_cartography_amd import fused
    seed, R, I, J, K, f, nbins, log_model, tile = case
    onebit = _onebit(case)
    d, (rn, rdS, rdC) = _explicit_ref(case)
    obs = _obs(d["Y"], d["Wx"], d["b"], d["sigma"], d["offset"], log_model, R, tile)
    assert obs.nnz == int(d["Wx"].sum())
    assert obs.desc.rowfmt == (1 if onebit else 0)
    if fmt == 0 and onebit:
        obs._fill(0)
    assert obs.desc.rowfmt == fmt
    S = d["S0"].cuda().requires_grad_(True)
    C = d["C0"].cuda().requires_grad_(True)
    nll = fused.ProbitNLL.apply(S, C, obs)
    nll.backward()
    P = I * J
    e_n = abs(nll.item() - rn) / abs(rn)
    e_s = rel_fro(S.grad.cpu().reshape(R, P).numpy(), rdS)
    e_c = rel_fro(C.grad.cpu().numpy(), rdC)
    print("case", case, "fmt", fmt, "nll", e_n, "dS", e_s, "dC", e_c)
    assert e_n < 1e-5
    assert e_s < 1e-5
    assert e_c < 1e-5


@pytest.mark.parametrize("seed,R,I,J,K,tile", [(61, 8, 96, 80, 256, None),
                                               (62, 16, 64, 64, 128, 512)])
def test_logit_signed_rows_match_code_field_entries(seed, R, I, J, K, tile):
    from quantized_spectrum_cartography_amd import qmc
    d = _random_case(seed, R, I, J, K)
    res = {}
    for fmt in (1, 0):
        o = _obs(d["Y"], d["Wx"], d["b"], d["sigma"], R=R, tile=tile)
        assert o.desc.rowfmt == 1, "the signed-row layout applies to one-bit logistic cases"
        if fmt == 0:
            o._fill(0)
        r = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], S_init=d["S0"], C_init=d["C0"],
                      max_iter=7, obs=o)
        assert o.desc.rowfmt == fmt
        res[fmt] = r
    assert np.array_equal(res[0].S.cpu().numpy(), res[1].S.cpu().numpy())
    assert np.array_equal(res[0].C.cpu().numpy(), res[1].C.cpu().numpy())
    assert np.allclose(res[0].costs_c, res[1].costs_c, rtol=1e-6, atol=0)
    assert np.allclose(res[0].costs_s, res[1].costs_s, rtol=1e-6, atol=0)


@pytest.mark.parametrize("seed,R,I,J,K,nbins,tile", [(42, 8, 96, 80, 256, 2, None),
                                                     (47, 6, 40, 56, 100, 5, 256)])
def test_logit_fused_spass_cpass_bitexact(seed, R, I, J, K, nbins, tile):
    """qsc_scpass reproduces qsc_spass mode 1 + qsc_cpass bit for bit under the logistic kinds."""
    from quantized_spectrum_cartography_amd import qmc
    d = _random_case(seed, R, I, J, K, nbins=nbins)
    kw = dict(S_init=d["S0"], C_init=d["C0"], max_iter=11, loss="logit", tile=tile)
    a = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], fuse=False, **kw)
    assert not a.fused
    for g in (False, True):
        b = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], fuse=True, use_graph=g, **kw)
        assert b.fused, "the fused S-step + C-pass launch did not run"
        assert np.array_equal(a.S.cpu().numpy(), b.S.cpu().numpy())
        assert np.array_equal(a.C.cpu().numpy(), b.C.cpu().numpy())
        assert a.costs_c == b.costs_c and a.costs_s == b.costs_s


def test_logit_pass_deterministic():
    from quantized_spectrum_cartography_amd import fused
    d = _random_case(11, 8, 64, 64, 128)
    obs = _obs(d["Y"], d["Wx"], d["b"], d["sigma"], R=8)
    outs = []
    for _ in range(3):
        S = d["S0"].cuda().requires_grad_(True)
        C = d["C0"].cuda().requires_grad_(True)
        nll = fused.ProbitNLL.apply(S, C, obs)
        nll.backward()
        outs.append((nll.item(), S.grad.cpu().numpy(), C.grad.cpu().numpy()))
    for o in outs[1:]:
        assert o[0] == outs[0][0]
        assert np.array_equal(o[1], outs[0][1]) and np.array_equal(o[2], outs[0][2])


# ---------------------------------------------------------------------------------------
# solver
# ---------------------------------------------------------------------------------------
def test_logit_solver_vs_golden(golden):
    from quantized_spectrum_cartography_amd import qmc
    g = golden("solve_logit_32")
    d = _gin(g)
    n = int(g["n_iter"])
    kw = dict(offset=d["offset"], log_model=d["log_model"], lambda_c=float(g["lam_c"]),
              lambda_s=float(g["lam_s"]), lr_c=5e-3, lr_s=1e-2, project_s=False, loss="logit")
    r1 = qmc.solve(d["Y"], d["Wx"], d["b"], d["s"], S_init=d["S0"], C_init=d["C0"], max_iter=1, **kw)
    assert rel_fro(r1.S.cpu().numpy(), g["S_it1"]) < 1e-5
    assert rel_fro(r1.C.cpu().numpy(), g["C_it1"]) < 1e-5
    rn = qmc.solve(d["Y"], d["Wx"], d["b"], d["s"], S_init=d["S0"], C_init=d["C0"], max_iter=n, **kw)
    assert rel_fro(rn.S.cpu().numpy(), g["S_it%d" % n]) < 1e-5
    assert rel_fro(rn.C.cpu().numpy(), g["C_it%d" % n]) < 1e-5
    assert np.allclose(rn.costs_c, g["costs_c"], rtol=1e-5)
    assert np.allclose(rn.costs_s, g["costs_s"], rtol=1e-5)


@pytest.mark.parametrize("log_model", [False, True])
def test_logit_solver_vs_explicit_and_graph(log_model):
    """Free-S solve at 32 x 32 x 16 against logit_ref's explicit fp64 solve; the hipGraph replay
    gives the eager run's bits."""
    from quantized_spectrum_cartography_amd import qmc
    R, I, J, K = 3, 32, 32, 16
    d = _random_case(81 + int(log_model), R, I, J, K, f=0.3, nbins=4 if log_model else 2,
                     log_model=log_model)
    P = I * J
    n = 5
    S, C, cc, cs = lr.explicit_solve(d["S0"].reshape(R, P).numpy(), d["C0"].numpy(),
                                     d["Y"].reshape(K, P).numpy(), d["Wx"].reshape(K, P).numpy(),
                                     d["b"].numpy(), d["sigma"], d["offset"], log_model, n_iter=n)
    kw = dict(S_init=d["S0"], C_init=d["C0"], max_iter=n, loss="logit", offset=d["offset"],
              log_model=log_model, project_s=False)
    a = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], **kw)
    assert rel_fro(a.S.cpu().reshape(R, P).numpy(), S) < 1e-5
    assert rel_fro(a.C.cpu().numpy(), C) < 1e-5
    assert np.allclose(a.costs_c, cc, rtol=1e-5)
    assert np.allclose(a.costs_s, cs, rtol=1e-5)
    b = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], use_graph=True, **kw)
    assert np.array_equal(a.S.cpu().numpy(), b.S.cpu().numpy())
    assert np.array_equal(a.C.cpu().numpy(), b.C.cpu().numpy())


def test_logit_solver_holdout_runs():
    from quantized_spectrum_cartography_amd import qmc
    d = _random_case(83, 3, 32, 32, 16, f=0.3)
    r = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], S_init=d["S0"], C_init=d["C0"],
                  max_iter=20, loss="logit", holdout=0.1, check_every=5, patience=10)
    assert len(r.holdout_nll) >= 1 and np.isfinite(np.asarray(r.holdout_nll, np.float64)).all()
    assert np.isfinite(r.S.cpu().numpy()).all() and np.isfinite(r.C.cpu().numpy()).all()


# ---------------------------------------------------------------------------------------
# tails, predicate, K-slab
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [1, 0])
def test_logit_tails_are_finite_and_exact(fmt):
    """One-bit, R = 2, 16 x 16 x 8, s small enough that |z| = |thr - t| / s reaches ~60: the NLL
    and both gradients are finite and within 1e-5 of the fp64 reference -- the stable form (linear
    tail of log P), where the probit kind saturates to P == 0.  No value the form needs is
    denormal: exp(-60) = 9e-27."""
    from quantized_spectrum_cartography_amd import fused
    R, I, J, K = 2, 16, 16, 8
    P = I * J
    gen = torch.Generator().manual_seed(90)
    S0 = torch.rand(R, 1, I, J, generator=gen)
    C0 = torch.rand(R, K, generator=gen)
    Th = lr.ro.get_tensor(S0, C0)
    thr = float(Th.median())
    s = float(np.float32(float((Th - thr).abs().max()) / 60.0))
    b = torch.tensor([0.0, thr, float(Th.max()) + 1.0])
    Y = torch.randint(0, 2, (K, 1, I, J), generator=gen)  # half the entries on the wrong side
    Wx = torch.ones(K, 1, I, J)
    z = (thr - Th) / s
    assert 55.0 < float(z.abs().max()) <= 60.5
    obs = _obs(Y, Wx, b, s, R=R)
    assert obs.desc.rowfmt == 1
    if fmt == 0:
        obs._fill(0)
    S = S0.cuda().requires_grad_(True)
    C = C0.cuda().requires_grad_(True)
    nll = fused.ProbitNLL.apply(S, C, obs)
    nll.backward()
    rn, rdS, rdC = lr.nll_grad(S0.reshape(R, P).numpy(), C0.numpy(), Y.reshape(K, P).numpy(),
                               Wx.reshape(K, P).numpy(), b.numpy(), s)
    assert np.isfinite(rn)
    assert np.isfinite(nll.item())
    assert torch.isfinite(S.grad).all() and torch.isfinite(C.grad).all()
    assert abs(nll.item() - rn) / abs(rn) < 1e-5
    assert rel_fro(S.grad.cpu().reshape(R, P).numpy(), rdS) < 1e-5
    assert rel_fro(C.grad.cpu().numpy(), rdC) < 1e-5


def test_logit_signed_rows_predicate():
    from quantized_spectrum_cartography_amd import _lib
    d1 = _random_case(66, 4, 32, 32, 64)
    o1 = _obs(d1["Y"], d1["Wx"], d1["b"], d1["sigma"], R=4)
    assert o1.model.loss == 2 and o1.desc.rowfmt == 1
    assert _lib.lib().qsc_obs_signed_rows_ok(o1.desc, 4, o1.model) == 1
    d5 = _random_case(67, 4, 32, 32, 64, nbins=5)
    o5 = _obs(d5["Y"], d5["Wx"], d5["b"], d5["sigma"], R=4)
    assert o5.desc.rowfmt == 0
    assert _lib.lib().qsc_obs_signed_rows_ok(o5.desc, 4, o5.model) == 0
    dl = _random_case(65, 4, 32, 32, 64, nbins=4, log_model=True)
    ol = _obs(dl["Y"], dl["Wx"], dl["b"], dl["sigma"], offset=dl["offset"], log_model=True, R=4)
    assert ol.desc.rowfmt == 0
    assert _lib.lib().qsc_obs_signed_rows_ok(ol.desc, 4, ol.model) == 0
    # a one-bit layout under the log model (two raw edges are not saturated): refused
    mlog = _lib.make_model(d1["b"], d1["sigma"], 1e-3, True, loss="logit")
    assert _lib.lib().qsc_obs_signed_rows_ok(o1.desc, 4, mlog) == 0


def test_logit_kslab_shards_sum_to_the_single_pass():
    """tests/test_gpu_kslab.py's smallest case (R = 3, 64 x 80 x 96, 256-position tiles) under
    loss="logit": qsc_cpass_nsq leaves the workspace exactly as qsc_cpass + qsc_slice_nsq (that
    file's bit-for-bit tolerance), and the K-slab S-passes (qsc_spass_kslab) of two bin slabs sum
    to the single-GPU S-pass -- gradient and NLL, to summation order (1e-6)."""
    from quantized_spectrum_cartography_amd import _lib
    from quantized_spectrum_cartography_amd.fused import PassEngine
    R, tile = 3, 256
    I, J, K = 64, 80, 96
    d = _random_case(94 + R, R, I, J, K)
    obs = _obs(d["Y"], d["Wx"], d["b"], d["sigma"], R=R, tile=tile)
    S = obs.to_positions(d["S0"].reshape(R, -1))
    C = d["C0"].reshape(R, -1).cuda().contiguous()
    a, b = PassEngine(obs, R), PassEngine(obs, R)
    a.cpass(S, C)
    a.slice_nsq(S)
    b.cpass_nsq(S, C)
    torch.cuda.synchronize()
    assert torch.equal(a.ws, b.ws)
    # single-GPU S-pass
    e = PassEngine(obs, R)
    e.init_state(S)
    dS = torch.empty_like(S)
    e.spass(S, C, 0, dS=dS)
    e.flush(record=False)
    nll = e.field("nll_s").item()
    # two K-slabs with the global pixel order, each through qsc_spass_kslab
    u = _lib.QSC_SLICE
    ns = obs.Pp // u
    world = 2
    cs = -(-ns // world)
    RP = S.shape[1]
    total = torch.zeros_like(S)
    nll_sum = 0.0
    for r in range(world):
        k0, k1 = r * K // world, (r + 1) * K // world
        o = _obs(d["Y"][k0:k1], d["Wx"][k0:k1], d["b"], d["sigma"], R=R, tile=tile, perm=obs.perm)
        eng = PassEngine(o, R)
        eng.init_state(S)
        Cl = C[:, k0:k1].contiguous()
        rs = torch.zeros(world, cs + 1, u, RP, device="cuda")
        eng.spass_kslab(S, Cl, rs, cs * u, world)
        eng.flush(record=False)
        nll_sum += eng.field("nll_s").item()
        nsq = torch.zeros(1, device="cuda")
        eng.sumsq(Cl, nsq)
        assert torch.equal(rs[:, cs, 0, 0], nsq.expand(world))  # ||C_slab||^2 rides along
        total += rs[:, :cs].reshape(world * cs * u, RP)[:obs.Pp]
    assert rel_fro(total.cpu().numpy(), dS.cpu().numpy()) < 1e-6
    assert abs(nll_sum - nll) / abs(nll) < 1e-6
