"""A numpy packer of a list of readings into the two sliced sparse formats, written from the
format description in include/qsc.h (qsc_obs_desc and the "Observation packing from a LIST of
readings" section) alone: pixel order by reading count, S-format slices of 32 positions,
C-format (tile, k-slice) blocks of 64 count-sorted bins over snake-dealt tile rows, 4-entry chunk
interleave, widths rounded to 4, code-field and signed-row values, pads, QSC_ENTRY_TAIL.  Lists
hold their readings in ascending k / qlocal, equal keys in input order.

Also the helpers the readings tests share: readings of a dense (Y, Wx), snapshot stacks, and a
decode of the packed lists back into per-pixel and per-(tile, bin) sequences."""
import numpy as np

SLICE, TAIL = 32, 256


def _up(x, m):
    return -(-x // m) * m


def entry_values(idx, code, rows, rowfmt, wide):
    if rowfmt == 1:
        return idx + np.where(code == 1, _up(rows, 16), 0)
    return idx | (code << (24 if wide else 12))


def pad_value(rows, rowfmt, wide):
    if rowfmt == 1:
        return 2 * _up(rows, 16)
    return (255 << 24) if wide else (15 << 12)


def tile_of(pos, nt):
    """(tile, qlocal) of positions: tile rows are whole slices dealt in snake order."""
    g, l = pos // SLICE, pos % SLICE
    i, r = g // nt, g % nt
    return np.where(i % 2 == 1, nt - 1 - r, r), i * SLICE + l


def pack(k, p, code, K, P, PT, nbins, rowfmt=0, perm=None):
    """-> dict of the arrays and descriptor fields of a packing, dtypes as on the device."""
    k, p, code = (np.asarray(a).astype(np.int64) for a in (k, p, code))
    n = k.size
    assert ((k >= 0) & (k < K) & (p >= 0) & (p < P) & (code >= 0) & (code < nbins)).all()
    Pp = _up(P, PT)
    nt, nks = Pp // PT, -(-K // 64)
    Kp, ns = nks * 64, Pp // SLICE
    wide = int(K > 4096 or PT > 4096 or nbins > 15)
    et = np.uint32 if wide else np.uint16
    cnt = np.bincount(p, minlength=P)
    if perm is None:
        perm = np.r_[np.argsort(-cnt, kind="stable"), -np.ones(Pp - P, dtype=np.int64)]
    perm = np.asarray(perm).astype(np.int64)
    iperm = np.full(P, -1, dtype=np.int64)
    iperm[perm[perm >= 0]] = np.nonzero(perm >= 0)[0]
    pos = iperm[p]
    assert (pos >= 0).all()
    # ---- S-format ----
    poscnt = np.bincount(pos, minlength=Pp)
    s_width = _up(poscnt.reshape(ns, SLICE).max(1), 4)
    s_off = np.r_[0, np.cumsum(s_width * SLICE)]
    s_ent = np.full(s_off[-1] + TAIL, pad_value(K, rowfmt, wide), dtype=np.int64)
    order = np.lexsort((k, pos))  # by (position, k), stable
    seg = np.r_[0, np.cumsum(poscnt)]
    ps = pos[order]
    j = np.arange(n) - seg[ps]
    s_ent[s_off[ps // SLICE] + (j // 4) * (SLICE * 4) + (ps % SLICE) * 4 + j % 4] = \
        entry_values(k[order], code[order], K, rowfmt, wide)
    # ---- C-format ----
    t, ql = tile_of(pos, nt)
    b = t * Kp + k
    ccount = np.bincount(b, minlength=nt * Kp).reshape(nt, Kp)
    ccount[:, K:] = -1  # padding bins come last
    kmap = np.argsort(-ccount, axis=1, kind="stable")
    kinv = np.empty_like(kmap)
    np.put_along_axis(kinv, kmap, np.broadcast_to(np.arange(Kp), kmap.shape), axis=1)
    first = np.take_along_axis(ccount, kmap[:, ::64], axis=1)  # each k-slice's longest list
    c_width = _up(np.maximum(first, 0), 4).reshape(-1)
    c_off = np.r_[0, np.cumsum(c_width * 64)]
    c_ent = np.full(c_off[-1] + TAIL, pad_value(PT, rowfmt, wide), dtype=np.int64)
    order = np.lexsort((ql, b))  # by (tile, bin, qlocal), stable
    seg = np.r_[0, np.cumsum(np.maximum(ccount, 0).reshape(-1))]
    bs = b[order]
    j = np.arange(n) - seg[bs]
    rank = kinv[t[order], k[order]]
    blk = t[order] * nks + rank // 64
    c_ent[c_off[blk] + (j // 4) * 256 + (rank % 64) * 4 + j % 4] = \
        entry_values(ql[order], code[order], PT, rowfmt, wide)
    return dict(counts=cnt.astype(np.int32), perm=perm.astype(np.int32),
                s_width=s_width.astype(np.int32), s_off=s_off.astype(np.int64),
                c_width=c_width.astype(np.int32), c_off=c_off.astype(np.int64),
                c_kmap=kmap.reshape(-1).astype(np.int32), s_entries=s_ent.astype(et),
                c_entries=c_ent.astype(et),
                desc=dict(K=K, P=P, Pp=Pp, PT=PT, ntiles=nt, nks=nks, wide=wide, nbins=nbins,
                          nnz=n, s_entries=s_ent.size, c_entries=c_ent.size, rowfmt=rowfmt))


def dense_readings(Y, Wx):
    """(k, p, code) int64 of the observed cells of a dense (K, ..., I, J) Y and mask Wx, in
    (k, p) order."""
    K = Y.shape[0]
    Yn = np.asarray(Y).reshape(K, -1)
    Wn = np.ones_like(Yn) if Wx is None else np.asarray(Wx).reshape(K, -1)
    kk, pp = np.nonzero(Wn != 0)
    return kk.astype(np.int64), pp.astype(np.int64), Yn[kk, pp].astype(np.int64)


def stack_readings(snapshots):
    """The concatenated readings of dense snapshots [(Y_m, Wx_m), ...]."""
    parts = [dense_readings(Y, Wx) for Y, Wx in snapshots]
    return tuple(np.concatenate([q[a] for q in parts]) for a in range(3))


def decode_values(v, rows, rowfmt, wide, nbins):
    """entry values -> (index, code, is_pad) (include/qsc.h)."""
    v = v.astype(np.int64)
    if rowfmt == 1:
        so = _up(rows, 16)
        pad = v >= 2 * so
        assert (v[pad] < 2 * so + 16).all()
        code = ((v >= so) & ~pad).astype(np.int64)
        return np.where(pad, 0, v - code * so), code, pad
    bits, padcode = (24, 255) if wide else (12, 15)
    idx, code = v & ((1 << bits) - 1), v >> bits
    pad = code == padcode
    assert (code[~pad] < nbins).all()
    return idx, code, pad


def decode_lists(a):
    """The packed lists of `a` (a dict as pack() returns) in slot order, pads dropped:
    ({pixel: [(k, code), ...]}, {(tile, bin): [(qlocal, code), ...]}).  Pads may stand anywhere in
    a list (a scheduled list interleaves them); padding positions and bins hold pads only."""
    d = a["desc"]
    K, PT, nt, nks = d["K"], d["PT"], d["ntiles"], d["nks"]
    s, c = a["s_entries"], a["c_entries"]
    per_pixel, per_bin = {}, {}
    for sl in range(d["Pp"] // SLICE):
        W = int(a["s_width"][sl])
        j = np.arange(W)
        for l in range(SLICE):
            pix = int(a["perm"][sl * SLICE + l])
            idx = a["s_off"][sl] + (j // 4) * (SLICE * 4) + l * 4 + j % 4
            kk, code, pad = decode_values(s[idx], K, d["rowfmt"], d["wide"], d["nbins"])
            got = list(zip(kk[~pad].tolist(), code[~pad].tolist()))
            if pix < 0:
                assert not got
            elif got:
                per_pixel[pix] = got
    for t in range(nt):
        for ks in range(nks):
            blk = t * nks + ks
            W = int(a["c_width"][blk])
            j = np.arange(W)
            for l in range(64):
                kb = int(a["c_kmap"][blk * 64 + l])
                idx = a["c_off"][blk] + (j // 4) * 256 + l * 4 + j % 4
                ql, code, pad = decode_values(c[idx], PT, d["rowfmt"], d["wide"], d["nbins"])
                got = list(zip(ql[~pad].tolist(), code[~pad].tolist()))
                if got:
                    assert kb < K
                    per_bin[(t, kb)] = got
    for ent, rows in ((s, K), (c, PT)):
        assert decode_values(ent[-TAIL:], rows, d["rowfmt"], d["wide"], d["nbins"])[2].all()
    return per_pixel, per_bin


def expected_lists(k, p, code, perm, PT):
    """What decode_lists must give for natural-order packing: every pixel's (k, code) in
    ascending k and every (tile, bin)'s (qlocal, code) in ascending qlocal, equal keys in input
    order."""
    k, p, code = (np.asarray(a).astype(np.int64) for a in (k, p, code))
    perm = np.asarray(perm).astype(np.int64)
    nt = perm.size // PT
    iperm = np.full(int(perm.max()) + 1, -1, dtype=np.int64)
    iperm[perm[perm >= 0]] = np.nonzero(perm >= 0)[0]
    t, ql = tile_of(iperm[p], nt)
    per_pixel, per_bin = {}, {}
    for e in np.lexsort((k, p)):
        per_pixel.setdefault(int(p[e]), []).append((int(k[e]), int(code[e])))
    for e in np.lexsort((ql, k, t)):
        per_bin.setdefault((int(t[e]), int(k[e])), []).append((int(ql[e]), int(code[e])))
    return per_pixel, per_bin
