"""GPU: the packed observation formats (qsc_obs_count, qsc_obs_order, qsc_obs_layout,
qsc_obs_fill, qsc_obs_schedule) decoded back on the host and compared with the dense codes.

The decode below is written from the format description in include/qsc.h alone (slice offsets,
4-entry chunk interleave, c_kmap, snake-dealt tile rows, code-field and signed-row values, pads,
the QSC_ENTRY_TAIL), not from the library's code: the passes are otherwise the only readers of
the packing, and a fill and a walk that agree on a wrong convention cancel each other there."""
import numpy as np
import pytest

from test_gpu_fused import _edge_mask, _random_case
from test_pass_matrix_host import TILE, WIDE_ONEBIT, data

pytestmark = pytest.mark.gpu

SLICE, TAIL, UNOBSERVED = 32, 256, 0xFF  # QSC_SLICE, QSC_ENTRY_TAIL, QSC_UNOBSERVED


def _up(x, m):
    return -(-x // m) * m


def _values(obs, v, rows):
    """Entry values of a table with `rows` rows -> (index, code, is_pad), by include/qsc.h."""
    d = obs.desc
    if d.rowfmt == 1:
        so = _up(rows, 16)
        pad = v >= 2 * so
        assert (v[pad] < 2 * so + 16).all(), "a signed-row pad is one of the rows 2 So + 0..15"
        code = ((v >= so) & ~pad).astype(np.int64)
        idx = np.where(pad, 0, v - code * so)
        return idx, code, pad
    bits, padcode = (24, 255) if d.wide else (12, 15)
    idx, code = v & ((1 << bits) - 1), v >> bits
    pad = code == padcode
    assert (code[~pad] < d.nbins).all()
    return idx, code, pad


def _host(obs):
    et = np.uint32 if obs.desc.wide else np.uint16
    return dict(s=obs.s_entries.cpu().numpy().view(et).astype(np.int64),
                c=obs.c_entries.cpu().numpy().view(et).astype(np.int64),
                s_width=obs.s_width.cpu().numpy(), s_off=obs.s_off.cpu().numpy(),
                c_width=obs.c_width.cpu().numpy(), c_off=obs.c_off.cpu().numpy(),
                kmap=obs.c_kmap.cpu().numpy().astype(np.int64),
                perm=obs.perm.cpu().numpy().astype(np.int64),
                codes=obs.codes.cpu().numpy())


def _tile_positions(t, PT, ntiles):
    """Position of every row qlocal of tile t: whole slices dealt in snake order."""
    ql = np.arange(PT)
    i = ql // SLICE
    g = i * ntiles + np.where(i % 2 == 1, ntiles - 1 - t, t)
    return g * SLICE + ql % SLICE


def _walk(ent, width, off, lanes, total):
    """Every (block, lane, j) slot of a format: yields (block, slot index array [lanes][W]) and
    checks that the blocks tile [0, total - TAIL) exactly, followed by the tail."""
    seen = np.zeros(total - TAIL, dtype=np.int32)
    blocks = []
    for b in range(len(width)):
        W = int(width[b])
        j = np.arange(W)
        idx = off[b] + (j // 4)[None, :] * (lanes * 4) + np.arange(lanes)[:, None] * 4 + (j % 4)[None, :]
        assert W == 0 or (idx.min() >= 0 and idx.max() < total - TAIL)
        np.add.at(seen, idx.ravel(), 1)
        blocks.append(idx)
    assert (seen == 1).all(), "the lists cover every entry before the tail exactly once"
    return blocks


def _expected(h, Kk, P):
    kk, pp = np.nonzero(h["codes"] != UNOBSERVED)
    return np.sort((kk.astype(np.int64) * P + pp) * 256 + h["codes"][kk, pp])


def check_packing(obs, natural_order):
    d = obs.desc
    h = _host(obs)
    Kk, P, Pp, PT = obs.K, obs.P, d.Pp, d.PT
    ntiles, nks = d.ntiles, d.nks
    observed = h["codes"] != UNOBSERVED
    # ---- descriptor ----
    assert (d.K, d.P, d.Pp, d.ntiles, d.nks) == (Kk, P, _up(P, PT), _up(P, PT) // PT, -(-Kk // 64))
    assert d.wide == int(Kk > 4096 or PT > 4096 or d.nbins > 15)
    assert d.nnz == int(observed.sum())
    assert d.s_entries == h["s"].size == h["s_off"][-1] + TAIL
    assert d.c_entries == h["c"].size == h["c_off"][-1] + TAIL
    # ---- pixel order: count-descending, stable; -1 on padding positions ----
    cnt = observed.sum(0)
    assert np.array_equal(obs.counts.cpu().numpy(), cnt)
    assert np.array_equal(h["perm"][:P], np.argsort(-cnt, kind="stable"))
    assert (h["perm"][P:] == -1).all() and h["perm"].size == Pp
    want = _expected(h, Kk, P)

    # ---- S-format: slice s, lane l -> position 32 s + l -> pixel perm[position] ----
    got = []
    blocks = _walk(h["s"], h["s_width"], h["s_off"], SLICE, h["s"].size)
    assert len(blocks) == Pp // SLICE
    for s, idx in enumerate(blocks):
        k, code, pad = _values(obs, h["s"][idx], Kk)
        assert (k < Kk).all(), "every entry, pads included, names a row of the table"
        pix = np.broadcast_to(h["perm"][s * SLICE + np.arange(SLICE)][:, None], k.shape)
        assert (pix[~pad] >= 0).all(), "padding positions hold pads only"
        got.append((k[~pad] * P + pix[~pad]) * 256 + code[~pad])
        if natural_order:  # qsc_obs_fill: ascending k, pads last
            key = np.where(pad, Kk, k)
            assert (np.diff(key, axis=1) >= 0).all()
            assert (np.diff(key, axis=1)[(~pad)[:, 1:]] > 0).all()
    assert np.array_equal(np.sort(np.concatenate(got)), want)
    _, _, pad = _values(obs, h["s"][-TAIL:], Kk)
    assert pad.all()

    # ---- C-format: tile t, k-slice ks, lane l -> bin c_kmap[(t nks + ks) 64 + l] ----
    got = []
    blocks = _walk(h["c"], h["c_width"], h["c_off"], 64, h["c"].size)
    assert len(blocks) == ntiles * nks and h["kmap"].size == ntiles * nks * 64
    for t in range(ntiles):
        pos = _tile_positions(t, PT, ntiles)
        assert pos.max() < Pp
        pix_of = h["perm"][pos]
        tcnt = np.zeros(nks * 64, dtype=np.int64)
        real = pix_of >= 0
        tcnt[:Kk] = observed[:, pix_of[real]].sum(1)
        km = h["kmap"][t * nks * 64:(t + 1) * nks * 64]
        # in-tile count descending, ties to the lower k (so the empty padding bins >= K are last)
        assert np.array_equal(km, np.argsort(-tcnt, kind="stable"))
        for ks in range(nks):
            idx = blocks[t * nks + ks]
            ql, code, pad = _values(obs, h["c"][idx], PT)
            assert (ql < PT).all()
            kb = np.broadcast_to(km[ks * 64:(ks + 1) * 64][:, None], ql.shape)
            assert (kb[~pad] < Kk).all(), "padding bins >= K are empty"
            pix = pix_of[ql]
            assert (pix[~pad] >= 0).all()
            got.append((kb[~pad] * P + pix[~pad]) * 256 + code[~pad])
            if natural_order:  # ascending qlocal, pads last
                key = np.where(pad, PT, ql)
                assert (np.diff(key, axis=1) >= 0).all()
                assert (np.diff(key, axis=1)[(~pad)[:, 1:]] > 0).all()
    assert np.array_equal(np.sort(np.concatenate(got)), want)
    _, _, pad = _values(obs, h["c"][-TAIL:], PT)
    assert pad.all()


def _observations(d, R, tile, schedule, loss="probit"):
    from quantized_spectrum_cartography_amd.obs import Observations
    return Observations(d["Y"], d["Wx"], d["b"], d["sigma"], offset=d["offset"],
                        log_model=d["log_model"], R_hint=R, tile=tile, schedule=schedule, loss=loss)


@pytest.mark.parametrize("schedule", [False, True])
@pytest.mark.parametrize("fmt", ["code-field", "signed-rows", "wide"])
def test_packing_round_trip(fmt, schedule):
    """25 x 23 pixels, K = 70, tile 128 (ragged P and K, five tiles, 65 padding positions), f =
    0.3: narrow code-field, signed-row and wide (17 bins) entries, in fill order and scheduled."""
    d = data(6, 0.3, "lin17" if fmt == "wide" else "lin2")
    obs = _observations(d, 6, TILE, schedule)
    assert (obs.desc.PT, obs.desc.Pp, obs.desc.ntiles, obs.desc.nks) == (TILE, 640, 5, 2)
    assert obs.desc.rowfmt == (0 if fmt == "wide" else 1)
    if fmt == "code-field":
        obs._fill(0)
    assert obs.desc.wide == (fmt == "wide") and obs.desc.rowfmt == (fmt == "signed-rows")
    if fmt == "wide":  # codes past the narrow format's 4-bit field are in play
        seen = np.unique(obs.codes.cpu().numpy())
        assert np.array_equal(seen, np.r_[np.arange(17), UNOBSERVED])
    check_packing(obs, natural_order=not schedule)


@pytest.mark.parametrize("schedule", [False, True])
def test_packing_round_trip_wide_by_K(schedule):
    """K = 4160 > 4096 at 16 x 16 pixels: wide one-bit entries, 65 k-slices, bin indices that
    need more than the narrow format's 12 bits."""
    d = data(3, None, "wide-by-K")
    obs = _observations(d, 3, WIDE_ONEBIT["wide-by-K"][3], schedule)
    assert obs.desc.wide == 1 and obs.desc.rowfmt == 0 and obs.desc.nks == 65
    check_packing(obs, natural_order=not schedule)


@pytest.mark.parametrize("schedule", [False, True])
def test_packing_round_trip_holes(schedule):
    """The "holes" mask of test_edge_masks_vs_oracle (640 pixels and three bins never observed,
    so whole position slices and bin lists are empty), 48 x 48, K = 130."""
    R, Ih, Jh, Kh = 8, 48, 48, 130
    d = _random_case(70 + R, R, Ih, Jh, Kh)
    d["Wx"] = _edge_mask("holes", Kh, Ih, Jh, 70 + Kh)
    obs = _observations(d, R, None, schedule)
    w = obs.s_width.cpu().numpy()
    assert (w == 0).any() and (w > 0).any()
    check_packing(obs, natural_order=not schedule)
