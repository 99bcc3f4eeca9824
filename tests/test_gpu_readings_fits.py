"""GPU: the second-order consumers -- qmc.confidence, fit_S, fit_C, fit_S_smooth -- on an
Observations packed from repeated readings, against the existing numpy references, unchanged, on
the equivalent dense problems of tests/readings_fit_ref.py: M K stacked bins with C tiled M times
(info_ref, sfit_ref, sfit_smooth_ref) and M P stacked pixels with S tiled (cfit_ref).

Shapes: tests/test_gpu_sfit.py's (9 x 15 pixels, tile 64, Pp = 192, R = 3 / 8 / 16, K = 37 / 70,
the five layouts / models of sfit_ref.CASES), M = 3 snapshots at sampling rate 0.7: a cell is read
0 to 3 times, a pixel's list holds up to 3 K entries (> K) and a (tile, bin) list up to 3 x 64
(> PT).  Pixel 0 is unobserved; on the C side bin 0 is.

Bounds: those the quantities have in tests/test_gpu_info.py, test_gpu_sfit.py, test_gpu_cfit.py
and test_gpu_sfit_smooth.py -- blocks rel_fro <= 1e-5; standard deviations and single steps within
max(1e-5, 10 floor); minimisers within 10 floor (and, for S, the fp64 gradient within 10 x that at
the fp32 reference's result) -- every floor the error of the fp32 numpy reference against the
fp64 one on the same stacked inputs, measured here.  tests/test_readings_host.py checks on the
CPU that the references converge on these inputs within their step limits."""
import numpy as np
import pytest
import torch

import cfit_ref as cr
import info_ref as ir
import readings_fit_ref as rf
import sfit_ref as sr
import sfit_smooth_ref as ssr
from conftest import rel_fro
from test_gpu_cfit import raw_fit as raw_cfit
from test_gpu_sfit import max_rel, raw_fit as raw_sfit
from test_gpu_sfit_smooth import visits

pytestmark = pytest.mark.gpu

P, TILE = rf.P, rf.TILE
_OBS, _REF = {}, {}


def observations(name, side):
    from quantized_spectrum_cartography_amd.obs import Observations
    key = (name, side)
    if key not in _OBS:
        d, _ = rf.problem(name)
        obs = Observations.from_readings(
            *rf.readings(name, side), (d["K"], rf.I, rf.J), d["b"], d["sigma"], offset=d["offset"],
            log_model=d["log_model"], tile=TILE, R_hint=d["R"], loss=d["loss"])
        assert obs.codes is None and obs.stats()["max_repeat"] == rf.M and obs.Pp == 192
        assert int(obs.counts.max()) > d["K"]  # a pixel list longer than K
        assert int(obs.c_width.max()) > obs.desc.PT  # a (tile, bin) list longer than the tile
        _OBS[key] = obs
    return _OBS[key]


def cached(key, fn):
    if key not in _REF:
        r = fn()
        for v in (r.values() if isinstance(r, dict) else [r]):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def near_s(d):
    return 0.8 * d["S"].reshape(d["R"], P).double().numpy()


def default_s(d):
    return (np.ones if d["log_model"] else np.zeros)((d["R"], P))


# ---- confidence -------------------------------------------------------------------------------
def ref_blocks(name, kind):
    d, _ = rf.problem(name)
    m = rf.stacked_bins(name)
    return cached(("blocks", name, kind), lambda: ir.blocks(
        d["S"].reshape(d["R"], P).double().numpy(), m["C"], m["Y"], m["Wx"], m["b"], m["sigma"],
        m["offset"], m["log_model"], m["loss"], kind))


@pytest.mark.parametrize("kind", ["expected", "observed"])
@pytest.mark.parametrize("name", rf.CASES)
def test_confidence_blocks_vs_stacked_bins(name, kind):
    from quantized_spectrum_cartography_amd import qmc
    d, _ = rf.problem(name)
    obs = observations(name, "s")
    c = qmc.confidence(obs, d["S"], d["C"], kind=kind, ridge=1.0)
    e = rel_fro(c.info.cpu().numpy(), ref_blocks(name, kind))
    print("readings", name, kind, "rowfmt", obs.desc.rowfmt, "info rel_fro", e)
    assert tuple(c.info.shape) == (P, d["R"], d["R"]) and (c.info[0] == 0).all()
    assert e <= 1e-5


@pytest.mark.parametrize("ridge", rf.RIDGES)
@pytest.mark.parametrize("kind", ["expected", "observed"])
@pytest.mark.parametrize("name", rf.CASES)
def test_confidence_standard_deviations_vs_stacked_bins(name, kind, ridge):
    from quantized_spectrum_cartography_amd import qmc
    d, _ = rf.problem(name)
    obs = observations(name, "s")
    R, K = d["R"], d["K"]
    Jr = ref_blocks(name, kind)
    C64 = d["C"].double().numpy()
    sS, sT, bad = ir.stds(Jr, C64, ridge)
    assert bad == 0
    fS, fT = ir.stds_fp32(Jr, C64, ridge)
    floor = max(ir.max_rel(fS, sS), ir.max_rel(fT, sT))
    tol = max(1e-5, 10 * floor)
    c = qmc.confidence(obs, d["S"], d["C"], kind=kind, ridge=ridge, map_std=True)
    eS = ir.max_rel(c.std_S.reshape(R, P).cpu().numpy(), sS)
    eT = ir.max_rel(c.std_T.reshape(K, P).cpu().numpy(), sT)
    print("readings", name, kind, "ridge", ridge, "std_S", eS, "std_T", eT, "floor", floor, "tol",
          tol)
    assert c.unidentified == 0
    assert eS <= tol
    assert eT <= tol


# ---- fit_S ------------------------------------------------------------------------------------
def sfit_reference(name, ridge, what, dtype, **kw):
    d, _ = rf.problem(name)
    m = rf.stacked_bins(name)
    S0 = near_s(d) if what == "near" else default_s(d)
    if dtype is None:
        return cached(("sfit", name, ridge, what), lambda: sr.minimise_fp64(S0, ridge=ridge, **m))
    return cached(("sfit", name, ridge, what, dtype, tuple(sorted(kw.items()))),
                  lambda: sr.fit(S0, ridge=ridge, dtype=dtype, **m, **kw))


@pytest.mark.parametrize("ridge", rf.RIDGES)
@pytest.mark.parametrize("name", rf.CASES)
def test_fit_s_one_step_vs_stacked_bins(name, ridge):
    d, _ = rf.problem(name)
    obs = observations(name, "s")
    o = sr.observed_pixels(rf.stacked_bins(name)["Wx"])
    r64 = sfit_reference(name, ridge, "near", np.float64, max_steps=1, mu0=0.0)
    r32 = sfit_reference(name, ridge, "near", np.float32, max_steps=1, mu0=0.0)
    floor = max_rel(r32["S"][:, o], r64["S"][:, o])
    tol = max(1e-5, 10 * floor)
    g = raw_sfit(obs, d, near_s(d), ridge, max_steps=1, mu0=0.0)
    e = max_rel(g["S"][:, o], r64["S"][:, o])
    print("readings", name, "ridge", ridge, "fit_S one step", e, "floor", floor, "tol", tol)
    assert not np.isnan(g["S"]).any() and (g["steps"][o] == 1).all()
    assert e <= tol


@pytest.mark.parametrize("ridge", rf.RIDGES)
@pytest.mark.parametrize("name", rf.CASES)
def test_fit_s_minimiser_vs_stacked_bins(name, ridge):
    from quantized_spectrum_cartography_amd import qmc
    d, _ = rf.problem(name)
    m = rf.stacked_bins(name)
    obs = observations(name, "s")
    o = sr.observed_pixels(m["Wx"])
    R = d["R"]
    mn = sfit_reference(name, ridge, "default", None)
    r32 = sfit_reference(name, ridge, "default", np.float32)
    floor = max_rel(r32["S"][:, o], mn["S"][:, o])
    g_floor = np.abs(sr.gradient_fp64(r32["S"], ridge=ridge, project=d["log_model"], **m)[:, o]).max()
    res = qmc.fit_S(obs, d["C"], ridge=ridge)
    S = res.S.reshape(R, P).double().cpu().numpy()
    e = max_rel(S[:, o], mn["S"][:, o])
    gn = np.abs(sr.gradient_fp64(S, ridge=ridge, project=d["log_model"], **m)[:, o]).max()
    print("readings", name, "ridge", ridge, "fit_S error", e, "floor", floor, "gradient", gn,
          "floor", g_floor, "steps max", int(res.steps.max()))
    assert torch.isfinite(res.S).all() and np.isfinite(res.nll)
    assert res.unconverged == 0
    assert res.unidentified == 0
    assert e <= 10 * floor
    assert gn <= 10 * g_floor
    f64, _, _ = sr.evaluate(S, ridge=0.0, kind="observed", **m)
    assert np.isclose(res.nll, f64.sum(), rtol=1e-5)


# ---- fit_C ------------------------------------------------------------------------------------
def cfit_reference(name, ridge, what, dtype, **kw):
    d, _ = rf.problem(name)
    C0 = 0.8 * d["C"].double().numpy() if what == "near" else cr.default_start(d)
    return cached(("cfit", name, ridge, what, dtype, tuple(sorted(kw.items()))),
                  lambda: cr.fit(C0, ridge=ridge, dtype=dtype, **rf.stacked_pixels(name), **kw))


@pytest.mark.parametrize("ridge", rf.RIDGES)
@pytest.mark.parametrize("name", rf.CASES)
def test_fit_c_one_step_vs_stacked_pixels(name, ridge):
    d, _ = rf.problem(name)
    obs = observations(name, "c")
    o = cr.observed_bins(rf.stacked_pixels(name)["Wx"])
    r64 = cfit_reference(name, ridge, "near", np.float64, max_steps=1, mu0=0.0)
    r32 = cfit_reference(name, ridge, "near", np.float32, max_steps=1, mu0=0.0)
    floor = max_rel(r32["C"][:, o], r64["C"][:, o])
    tol = max(1e-5, 10 * floor)
    g = raw_cfit(obs, d, 0.8 * d["C"].double().numpy(), ridge, max_steps=1, mu0=0.0)
    e = max_rel(g["C"][:, o], r64["C"][:, o])
    print("readings", name, "ridge", ridge, "fit_C one step", e, "floor", floor, "tol", tol)
    assert not np.isnan(g["C"]).any() and (g["steps"][o] == 1).all()
    assert e <= tol


@pytest.mark.parametrize("ridge", rf.RIDGES)
@pytest.mark.parametrize("name", rf.CASES)
def test_fit_c_minimiser_and_std_c_vs_stacked_pixels(name, ridge):
    from quantized_spectrum_cartography_amd import qmc
    d, _ = rf.problem(name)
    m = rf.stacked_pixels(name)
    obs = observations(name, "c")
    o = cr.observed_bins(m["Wx"])
    mn = cfit_reference(name, ridge, "default", np.float64, max_steps=300, tol=1e-12)
    r32 = cfit_reference(name, ridge, "default", np.float32, max_steps=cr.MAX_STEPS)
    floor = max_rel(r32["C"][:, o], mn["C"][:, o])
    res = qmc.fit_C(obs, d["S"], ridge=ridge, max_steps=cr.MAX_STEPS, std=True)
    C = res.C.double().cpu().numpy()
    e = max_rel(C[:, o], mn["C"][:, o])
    print("readings", name, "ridge", ridge, "fit_C error", e, "floor", floor, "steps max",
          int(res.steps.max()))
    assert torch.isfinite(res.C).all() and np.isfinite(res.nll) and (res.C >= 0).all()
    assert res.unconverged == 0 and res.unidentified == 0
    assert e <= 10 * floor
    assert (C[(mn["C"] == 0) & o[None, :]] == 0).all()
    f64, _, _ = cr.evaluate(C, ridge=0.0, kind="observed", **m)
    assert np.isclose(res.nll, f64.sum(), rtol=1e-5)
    kind = sr.default_kind(d["log_model"])
    s64 = cr.std_fp64(C, kind=kind, ridge=ridge, **m)
    s32 = cr.std_fp64(C, kind=kind, ridge=ridge, dtype=np.float32, **m)
    sfloor = max_rel(s32, s64)
    stol = max(1e-5, 10 * sfloor)
    es = max_rel(res.std_C.double().cpu().numpy(), s64)
    print("readings", name, "ridge", ridge, "std_C error", es, "floor", sfloor, "tol", stol)
    assert torch.isfinite(res.std_C).all()
    assert es <= stol


# ---- fit_S_smooth -----------------------------------------------------------------------------
def ref_visits(name, ridge, dtype, kind, delta):
    d, _ = rf.problem(name)

    def run():
        s = near_s(d)
        for c in (0, 1):
            s = ssr.visit(s, c, rf.I, rf.J, rf.stacked_bins(name), ssr.WEIGHT, kind, delta,
                          ridge=ridge, inner_steps=1, dtype=dtype)["S"]
        return np.asarray(s, np.float64)
    return cached(("visits", name, ridge, dtype, kind), run)


@pytest.mark.parametrize("kind,delta", ssr.KINDS)
@pytest.mark.parametrize("ridge", rf.RIDGES)
@pytest.mark.parametrize("name", rf.CASES)
def test_fit_s_smooth_one_visit_per_colour_vs_stacked_bins(name, ridge, kind, delta):
    d, _ = rf.problem(name)
    obs = observations(name, "s")
    r64 = ref_visits(name, ridge, np.float64, kind, delta)
    r32 = ref_visits(name, ridge, np.float32, kind, delta)
    floor = ssr.pixel_rel(r32, r64)
    tol = max(1e-5, 10 * floor)
    g = visits(obs, d, near_s(d), (0, 1), ridge, kind=kind, delta=delta)
    e = ssr.pixel_rel(g["S"], r64)
    print("readings", name, "ridge", ridge, kind, "two visits", e, "floor", floor, "tol", tol)
    assert not np.isnan(g["S"]).any() and (g["steps"] == 1).all()
    assert e <= tol
    assert g["counters"][:, 2].sum() == 0
