"""GPU: per-pixel confidence from Fisher information -- qsc_sinfo, qsc_info_std, qsc_entry_info,
qmc.confidence and solve(confidence=...) -- against the fp64 reference of tests/info_ref.py.

Shapes: I x J = 9 x 15 (P = 135) with tile 64: Pp = 192, three tiles, six slices, 57 padding
positions; K = 37 (no multiple of 4) at R = 3 and R = 8, K = 70 at R = 16; pixel 0 unobserved;
sampling rate 0.7.  The smallest shapes with several slices and tiles, padding positions, list
pads, every rank template and both lane halves of a position.  Inputs: S ~ U(0.2, 1),
C ~ U(0.1, 1), one-bit thresholds near the map's median (0.9, 1.8, 3.5 at R = 3, 8, 16).

Tolerances: blocks at the project's pass tolerance, rel_fro <= 1e-5 (tests/test_gpu_fullsize.py);
standard deviations within max(1e-5, 10 floor), floor the error of an fp32 numpy Cholesky inverse
of the fp32-rounded reference blocks against fp64, measured in the test (the factor 10 allows for
the blocks' own fp32 summation error amplified by the condition number: with these draws at most
34 / 276 / 1110 at R = 3 / 8 / 16 and ridge 1e-2, floor <= 2.0e-6; DESIGN.md section 7k has the
measured errors)."""
import ctypes

import numpy as np
import pytest
import torch

import info_ref as ir
from conftest import rel_fro
from oracle import reference_ops as ro

pytestmark = pytest.mark.gpu

I, J, TILE = 9, 15, 64
P = I * J
RATE = 0.7

# name: (R, K, model, threshold, sigma, loss, seed)
CASES = {
    "onebit3": (3, 37, "onebit", 0.9, 0.4, "probit", 11),
    "onebit8": (8, 37, "onebit", 1.8, 0.6, "probit", 12),
    "onebit16": (16, 70, "onebit", 3.5, 0.8, "probit", 13),
    "log4": (8, 37, "log4", None, 0.5, "probit", 14),
    "logit": (16, 70, "onebit", 3.5, 0.5, "logit", 15),
    "logit_log4": (3, 37, "log4", None, 0.4, "logit", 16),
    "bins16": (3, 37, "bins16", None, 0.3, "probit", 17),
}
KINDS = ["expected", "observed"]

_PROB, _REF, _OBS = {}, {}, {}


def problem(name):
    """Inputs of a case (CPU tensors), built once."""
    if name in _PROB:
        return _PROB[name]
    R, K, model, thr, sigma, loss, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    S = 0.2 + 0.8 * torch.rand(R, 1, I, J, generator=g)
    C = 0.1 + 0.9 * torch.rand(R, K, generator=g)
    T = ro.get_tensor(S, C)
    if loss == "logit":
        u = torch.rand(T.shape, generator=g)
        noise = torch.log(u) - torch.log1p(-u)
    else:
        noise = torch.randn(T.shape, generator=g)
    offset, log_model = 0.0, False
    if model == "onebit":
        b = torch.tensor([0.0, thr, float(T.max()) + 1.0])
    elif model == "bins16":
        b = torch.quantile(T.reshape(-1), torch.linspace(0, 1, 17))
    else:
        offset, log_model = 1e-3, True
        x = torch.log(T + offset).reshape(-1)
        q = torch.quantile(x, torch.tensor([0.25, 0.5, 0.75]))
        b = torch.tensor([-23.025850296020508, float(q[0]), float(q[1]), float(q[2]),
                          float(x.max()) + 0.5])
    Y = ro.quantize(T, sigma, b, offset=offset, log_model=log_model, noise=noise).unsqueeze(1)
    Wx = torch.bernoulli(torch.full((K, 1, I, J), RATE), generator=g)
    Wx[:, :, 0, 0] = 0  # pixel 0 is unobserved
    d = dict(name=name, R=R, K=K, S=S, C=C, Y=Y, Wx=Wx, b=b, sigma=sigma, offset=offset,
             log_model=log_model, loss=loss, nbins=len(b) - 1)
    _PROB[name] = d
    return d


def ref_blocks(name, kind):
    """(P, R, R) fp64 reference blocks, computed once per (case, kind) and left unchanged."""
    key = (name, kind)
    if key not in _REF:
        d = problem(name)
        _REF[key] = ir.blocks(d["S"].reshape(d["R"], -1).double().numpy(), d["C"].double().numpy(),
                              d["Y"].reshape(d["K"], -1).numpy(), d["Wx"].reshape(d["K"], -1).numpy(),
                              d["b"].double().numpy(), d["sigma"], d["offset"], d["log_model"],
                              d["loss"], kind)
        _REF[key].setflags(write=False)
    return _REF[key]


def observations(name, schedule=None):
    from quantized_spectrum_cartography_amd.obs import Observations
    key = (name, schedule)
    if key not in _OBS:
        d = problem(name)
        _OBS[key] = Observations(d["Y"], d["Wx"], d["b"], d["sigma"], offset=d["offset"],
                                 log_model=d["log_model"], tile=TILE, R_hint=d["R"], loss=d["loss"],
                                 schedule=schedule)
    return _OBS[key]


def raw_blocks(obs, d, kind, layout=None):
    """qsc_sinfo through the ABI into a NaN-filled J (Pp, RP, RP): every element must be written."""
    from quantized_spectrum_cartography_amd import _lib, qmc
    R = d["R"]
    desc, s_entries, _ = layout or obs.layout(R)
    RP = obs.rank_pad(R)
    S_pos = obs.to_positions(d["S"].reshape(R, -1))
    Cd = d["C"].cuda().contiguous()
    Jb = torch.full((obs.Pp, RP, RP), float("nan"), device="cuda")
    _lib.call("qsc_sinfo", desc, _lib.ptr(s_entries), _lib.ptr(obs.s_width), _lib.ptr(obs.s_off),
              obs.model, R, _lib.ptr(S_pos), _lib.ptr(Cd), qmc.INFO_KINDS[kind], _lib.ptr(Jb),
              _lib.stream())
    return Jb


# ---------------------------------------------------------------------------------------
# (i) information blocks
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(CASES))
def test_info_blocks_vs_reference(name, kind):
    from quantized_spectrum_cartography_amd import qmc
    d = problem(name)
    obs = observations(name)
    R = d["R"]
    assert obs.Pp == 192 and obs.desc.ntiles == 3 and obs.Pp // 32 == 6
    assert bool(obs.desc.wide) == (d["nbins"] > 15)
    if name == "onebit3":
        assert obs.desc.rowfmt == 1, "the one-bit linear case is meant to run on signed rows"
    Jr = ref_blocks(name, kind)
    c = qmc.confidence(obs, d["S"], d["C"], kind=kind, ridge=1.0)
    assert tuple(c.info.shape) == (P, R, R) and c.std_T is None
    e = rel_fro(c.info.cpu().numpy(), Jr)
    print("case", name, kind, "rowfmt", obs.desc.rowfmt, "wide", obs.desc.wide, "info rel_fro", e)
    assert e <= 1e-5
    # the raw blocks: all written; padding rows / columns, padding positions and the unobserved
    # pixel exactly zero; symmetric bit for bit
    Jb = raw_blocks(obs, d, kind)
    assert not torch.isnan(Jb).any()
    assert torch.equal(Jb, Jb.transpose(1, 2))
    assert (Jb[:, R:, :] == 0).all() and (Jb[:, :, R:] == 0).all()
    pads = obs.perm < 0
    assert int(pads.sum()) == obs.Pp - P == 57
    assert (Jb[pads] == 0).all()
    assert (c.info[0] == 0).all()
    assert torch.equal(Jb[obs.iperm().long()][:, :R, :R], c.info)
    if kind == "expected":
        assert (torch.diagonal(c.info, dim1=1, dim2=2) >= 0).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["onebit3", "logit"])
def test_info_blocks_code_field_layout(name, kind, monkeypatch):
    """The one-bit linear models again through code-field entries (QSC_SIGNED_ROWS=0 in a fresh
    Observations): the same blocks up to summation order."""
    from quantized_spectrum_cartography_amd import qmc
    from quantized_spectrum_cartography_amd.obs import Observations
    d = problem(name)
    monkeypatch.setenv("QSC_SIGNED_ROWS", "0")
    obs = Observations(d["Y"], d["Wx"], d["b"], d["sigma"], tile=TILE, R_hint=d["R"],
                       loss=d["loss"])
    assert obs.desc.rowfmt == 0 and not obs.desc.wide
    c = qmc.confidence(obs, d["S"], d["C"], kind=kind)
    e = rel_fro(c.info.cpu().numpy(), ref_blocks(name, kind))
    print("case", name, kind, "code-field info rel_fro", e)
    assert e <= 1e-5


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(CASES))
def test_entry_information_vs_reference(name, kind):
    from quantized_spectrum_cartography_amd import utils
    d = problem(name)
    K, R = d["K"], d["R"]
    T = ro.get_tensor(d["S"], d["C"]).reshape(K, P)
    Y = d["Y"].reshape(K, P)
    h = utils.entry_information(T.cuda(), Y.cuda(), d["b"], d["sigma"], offset=d["offset"],
                                log_model=d["log_model"], loss=d["loss"], kind=kind)
    hr = ir.curvature(T.double().numpy(), Y.numpy(), d["b"].double().numpy(), d["sigma"],
                      d["offset"], d["log_model"], d["loss"], kind)
    e = rel_fro(h.cpu().numpy(), hr)
    print("case", name, kind, "entry rel_fro", e, "R", R)
    assert h.shape == T.shape and torch.isfinite(h).all()
    assert e <= 1e-5
    if kind == "expected":
        assert (h >= 0).all()


# ---------------------------------------------------------------------------------------
# (ii) standard deviations
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ridge", [1e-2, 1e-1, 1.0])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["onebit3", "onebit8", "onebit16"])
def test_standard_deviations_vs_reference(name, kind, ridge):
    from quantized_spectrum_cartography_amd import qmc
    d = problem(name)
    obs = observations(name)
    R, K = d["R"], d["K"]
    Jr = ref_blocks(name, kind)
    C64 = d["C"].double().numpy()
    sS, sT, bad = ir.stds(Jr, C64, ridge)
    assert bad == 0, "every block is positive definite with the ridge"
    # the fp32 floor, independent of the code under test
    fS, fT = ir.stds_fp32(Jr, C64, ridge)
    floor = max(ir.max_rel(fS, sS), ir.max_rel(fT, sT))
    tol = max(1e-5, 10 * floor)
    c = qmc.confidence(obs, d["S"], d["C"], kind=kind, ridge=ridge, map_std=True)
    assert tuple(c.std_S.shape) == (R, 1, I, J) and tuple(c.std_T.shape) == (K, 1, I, J)
    eS = ir.max_rel(c.std_S.reshape(R, P).cpu().numpy(), sS)
    eT = ir.max_rel(c.std_T.reshape(K, P).cpu().numpy(), sT)
    print("case", name, kind, "ridge", ridge, "std_S", eS, "std_T", eT, "floor", floor, "tol", tol)
    assert c.unidentified == 0
    assert eS <= tol
    assert eT <= tol
    # the unobserved pixel has only the ridge
    assert torch.allclose(c.std_S[:, 0, 0, 0], torch.full((R,), ridge ** -0.5, device="cuda"),
                          rtol=1e-6)


# ---------------------------------------------------------------------------------------
# (iii) unidentified positions
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["onebit3", "onebit8", "onebit16"])
def test_unobserved_pixel_is_unidentified_without_ridge(name, kind):
    from quantized_spectrum_cartography_amd import qmc
    d = problem(name)
    obs = observations(name)
    R, K = d["R"], d["K"]
    c = qmc.confidence(obs, d["S"], d["C"], kind=kind, ridge=0.0, map_std=True)
    inf = float("inf")
    assert (c.std_S[:, 0, 0, 0] == inf).all()
    assert (c.std_T[:, 0, 0, 0] == inf).all()
    assert c.unidentified >= 1
    assert not torch.isnan(c.std_S).any() and not torch.isnan(c.std_T).any()
    assert not torch.isnan(c.info).any()
    # padding positions are not counted: the count is that of the reference's non-PD blocks
    # (pixels without observations; every observed pixel has ~0.7 K >= R entries)
    _, _, bad = ir.stds(ref_blocks(name, kind), d["C"].double().numpy(), 0.0, map_std=False)
    nobs0 = int((d["Wx"].reshape(K, P).sum(dim=0) == 0).sum())
    assert bad == nobs0 >= 1
    assert c.unidentified == bad
    assert int(torch.isinf(c.std_S).any(dim=0).sum()) == bad


# ---------------------------------------------------------------------------------------
# (iv) determinism, list order
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("onebit8", "expected"), ("bins16", "observed"),
                                       ("logit", "observed")])
def test_two_calls_are_bit_identical_and_list_order_does_not_matter(name, kind):
    from quantized_spectrum_cartography_amd import qmc
    d = problem(name)
    obs = observations(name)
    a = qmc.confidence(obs, d["S"], d["C"], kind=kind, ridge=0.1, map_std=True)
    b = qmc.confidence(obs, d["S"], d["C"], kind=kind, ridge=0.1, map_std=True)
    assert torch.equal(a.info, b.info)
    assert torch.equal(a.std_S, b.std_S) and torch.equal(a.std_T, b.std_T)
    assert a.unidentified == b.unidentified == 0
    assert obs.schedule
    nat = observations(name, schedule=False)
    assert not nat.schedule
    n = qmc.confidence(nat, d["S"], d["C"], kind=kind, ridge=0.1)
    e = rel_fro(n.info.cpu().numpy(), a.info.cpu().numpy())
    print("case", name, kind, "natural list order vs scheduled", e)
    assert e <= 1e-5
    assert rel_fro(n.std_S.cpu().numpy(), a.std_S.cpu().numpy()) <= 1e-5


# ---------------------------------------------------------------------------------------
# (v) solve(confidence=...)
# ---------------------------------------------------------------------------------------
def test_solve_confidence_matches_confidence_and_leaves_the_solve_unchanged():
    from quantized_spectrum_cartography_amd import qmc
    d = problem("onebit3")
    R, K = d["R"], d["K"]
    g = torch.Generator().manual_seed(5)
    S0 = 0.2 + 0.5 * torch.rand(R, 1, I, J, generator=g)
    C0 = 0.1 + 0.5 * torch.rand(R, K, generator=g)
    kw = dict(S_init=S0, C_init=C0, max_iter=3, tile=TILE)
    args = (d["Y"], d["Wx"], d["b"], d["sigma"])
    plain = qmc.solve(*args, **kw)
    assert plain.std_S is None and plain.unidentified is None
    res = qmc.solve(*args, confidence="expected", **kw)
    assert torch.equal(res.S, plain.S) and torch.equal(res.C, plain.C)
    assert res.costs_c == plain.costs_c and res.costs_s == plain.costs_s
    assert res.fused == plain.fused
    obs = observations("onebit3")
    ridge = qmc.default_confidence_ridge(res.S, 100.0)
    assert ridge == 100.0 / float(torch.linalg.norm(res.S))
    c = qmc.confidence(obs, res.S, res.C, kind="expected", ridge=ridge)
    assert tuple(res.std_S.shape) == (R, 1, I, J)
    assert torch.equal(res.std_S, c.std_S)
    assert res.unidentified == c.unidentified == 0
    assert torch.isfinite(res.std_S).all()
    # an explicit ridge, and the holdout path
    r2 = qmc.solve(*args, confidence="observed", confidence_ridge=0.5, **kw)
    c2 = qmc.confidence(obs, r2.S, r2.C, kind="observed", ridge=0.5)
    assert torch.equal(r2.std_S, c2.std_S)
    r3 = qmc.solve(*args, confidence="expected", holdout=0.2, check_every=1, patience=2, **kw)
    assert tuple(r3.std_S.shape) == (R, 1, I, J) and torch.isfinite(r3.std_S).all()
    assert r3.unidentified == 0


# ---------------------------------------------------------------------------------------
# (vi) the ABI's argument checks
# ---------------------------------------------------------------------------------------
def test_abi_rejects_what_it_cannot_compute():
    from quantized_spectrum_cartography_amd import _lib
    from quantized_spectrum_cartography_amd.obs import Observations, ctypes_copy
    L = _lib.lib()
    d = problem("onebit3")
    R = d["R"]
    obs = observations("onebit3")
    desc, s_entries, _ = obs.layout(R)
    S_pos = obs.to_positions(d["S"].reshape(R, -1))
    Cd = d["C"].cuda().contiguous()
    Jb = torch.zeros((obs.Pp, 4, 4), device="cuda")
    p = _lib.ptr

    def sinfo(desc_=desc, model=obs.model, R_=R, kind=0, ent=s_entries):
        return L.qsc_sinfo(desc_, p(ent), p(obs.s_width), p(obs.s_off), model, R_, p(S_pos), p(Cd),
                           kind, p(Jb), None)

    assert sinfo() == 0
    # the squared loss is not a likelihood
    sq = Observations(d["Y"], d["Wx"], d["b"], d["sigma"], tile=TILE, R_hint=R, loss="squared")
    dsq, esq, _ = sq.layout(R)
    assert sq.model.loss == _lib.LOSSES["squared"]
    assert sinfo(desc_=dsq, model=sq.model, ent=esq) == _lib.QSC_EINVAL
    assert sinfo(kind=2) == _lib.QSC_EINVAL
    assert sinfo(R_=0) == _lib.QSC_EINVAL and sinfo(R_=17) == _lib.QSC_EINVAL
    m4 = _lib.make_model([0.0, 1.0, 2.0, 3.0], 0.4)  # bins of the model != bins of the layout
    assert sinfo(model=m4) == _lib.QSC_EINVAL
    # C^T beyond the LDS: K = 4096 rows of 20 floats at rank 16 (refused before any launch)
    big = _lib.QscObsDesc()
    ctypes_copy(big, desc)
    big.K, big.rowfmt = 4096, 0
    assert sinfo(desc_=big, R_=16) == _lib.QSC_EUNSUPPORTED
    # qsc_info_std / qsc_entry_info
    std = torch.zeros((obs.Pp, 4), device="cuda")
    nbad = torch.zeros(1, dtype=torch.int32, device="cuda")

    def info_std(ridge=0.1, R_=R, nb=nbad):
        return L.qsc_info_std(p(Jb), p(obs.perm), R_, obs.P, obs.Pp, p(Cd), obs.K,
                              ctypes.c_float(ridge), p(std), None, p(nb), None)

    assert info_std() == 0
    assert info_std(ridge=-1.0) == _lib.QSC_EINVAL
    assert info_std(ridge=float("nan")) == _lib.QSC_EINVAL
    assert info_std(R_=17) == _lib.QSC_EINVAL
    assert info_std(nb=None) == _lib.QSC_EINVAL
    Y = torch.zeros(8, dtype=torch.int64, device="cuda")
    T = torch.ones(8, device="cuda")
    H = torch.zeros(8, device="cuda")
    assert L.qsc_entry_info(p(Y), p(T), 8, obs.model, 1, p(H), None) == 0
    assert L.qsc_entry_info(p(Y), p(T), 8, sq.model, 1, p(H), None) == _lib.QSC_EINVAL
    assert L.qsc_entry_info(p(Y), p(T), 8, obs.model, 3, p(H), None) == _lib.QSC_EINVAL
    torch.cuda.synchronize()
