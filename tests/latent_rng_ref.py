"""Restatement of the generators' device latent stream (include/gode.h) in NumPy, on tests/wgan_ref.py's
Philox, for tests/test_host_latent_rng.py and tests/test_gpu_latent_rng.py: the counters and words exactly, the normals in
float64, Floyd's selection with Python integers.
"""
import numpy as np

import wgan_ref as W

MASK = 0xFFFFFFFF
CONTENT, MOTION, CLASS, SELECT = 0, 1, 2, 3


def tag(stream, field):
    """The third counter word: 0x60000000 | stream << 8 | field, stream < 2^21."""
    assert 0 <= int(stream) < (1 << 21) and 0 <= int(field) < 256
    return 0x60000000 | (int(stream) << 8) | int(field)


def counters(stream, field, call, e):
    """The Philox counter of each element index e: (q low word, call, tag, q high word), q = e >> 2."""
    q = np.asarray(e, dtype=np.uint64) >> np.uint64(2)
    return np.stack([q & np.uint64(MASK), np.full_like(q, int(call) & MASK), np.full_like(q, tag(stream, field)),
                     q >> np.uint64(32)], -1)


def words(seed, stream, field, call, e):
    """The word of every element index in e (any shape): lane e & 3 of its quad."""
    e = np.asarray(e, dtype=np.uint64)
    quads = W.philox4x32_10(counters(stream, field, call, e.reshape(-1)), W.seed_key(seed))
    lane = (e.reshape(-1) & np.uint64(3)).astype(np.int64)
    return np.asarray(quads, dtype=np.uint64)[np.arange(lane.size), lane].astype(np.uint32).reshape(e.shape)


def normals(seed, stream, field, call, e):
    """float64 Box-Muller of the elements in e: lanes 0 / 1 = r0 cos 2 pi u1, r0 sin 2 pi u1, lanes 2 / 3 from (u2, u3)."""
    e = np.asarray(e, dtype=np.uint64)
    flat = e.reshape(-1)
    quads = np.asarray(W.philox4x32_10(counters(stream, field, call, flat), W.seed_key(seed)), dtype=np.uint64)
    u = W.uniforms(quads.astype(np.uint32))
    lane = (flat & np.uint64(3)).astype(np.int64)
    idx = np.arange(lane.size)
    pair = (lane >> 1) * 2
    r = np.sqrt(-2.0 * np.log(u[idx, pair]))
    ang = 2.0 * np.pi * u[idx, pair + 1]
    return np.where(lane & 1, r * np.sin(ang), r * np.cos(ang)).reshape(e.shape)


def classes(seed, stream, call, g, C):
    """cls = umulhi(word of element g of field 2, C)"""
    w = words(seed, stream, CLASS, call, g).astype(np.uint64)
    return ((w * np.uint64(C)) >> np.uint64(32)).astype(np.int32)


def selection(seed, stream, call, B, R):
    """B distinct rows of range(R) by Floyd's algorithm on the words of field 3, sorted ascending."""
    assert 1 <= B <= R < (1 << 31)
    w = words(seed, stream, SELECT, call, np.arange(B, dtype=np.uint64))
    taken = set()
    for m in range(B):
        j = R - B + m
        t = (int(w[m]) * (j + 1)) >> 32
        taken.add(j if t in taken else t)
    return np.array(sorted(taken), dtype=np.int64)


def draw(seed, stream, call, n, outer, inner, T, n_all, C, traj0=0):
    """The four sub-blocks of one call: x float64 [outer, n, inner], content float64 [n, 50], sel_t int32 [n] (None in full
    mode: n_all == 0), cls int32 [n] (None when C == 0)."""
    sel_t = None
    if n_all > 0:
        rows = selection(seed, stream, call, n, n_all * T)
        g = traj0 + rows // T
        sel_t = (rows % T).astype(np.int32)
    else:
        g = traj0 + np.arange(n, dtype=np.int64)
    g = g.astype(np.uint64)
    XW = outer * inner
    content = normals(seed, stream, CONTENT, call, g[:, None] * np.uint64(50) + np.arange(50, dtype=np.uint64)[None, :])
    k = np.arange(XW, dtype=np.uint64)
    flat = normals(seed, stream, MOTION, call, g[:, None] * np.uint64(XW) + k[None, :])      # [n, outer*inner]
    x = np.ascontiguousarray(flat.reshape(n, outer, inner).transpose(1, 0, 2))
    cls = classes(seed, stream, call, g, C) if C > 0 else None
    return x, content, sel_t, cls
