"""swc_dtw of include/swc_mcd.h restated in numpy int64, vectorised over anti-diagonals: THE reference of tests/test_mcd_cpu.py
and tests/test_mcd_gpu.py (and the host yardstick of tools/bench_mcd.py).  Nothing here imports the package.

    r = dtw(x, y, band=0, mode=WARP)       x f32 [Tx][D], y f32 [Ty][D]
    r["total"] int, r["info"] int32 [4] = N, Tx, Ty, e, r["mean"] np.float32, r["path"] int32 [N][2]
"""
import numpy as np

WARP, DIAGONAL = 0, 1
MODES = {"warp": WARP, "diagonal": DIAGONAL}
MAX_FRAMES, MAX_D, QBITS, NBITS = 8192, 32, 13, 14
QMAX = (1 << QBITS) - 1
INF = np.int64(1) << np.int64(62)          # the key of a cell that is not allowed or not reachable
D_MAX = int(np.floor(np.sqrt(256.0 * MAX_D * (2 * QMAX) ** 2)))


def peak_of(x, y):
    """the bit pattern maximum of |v| over both sides (uint32); 0 for two empty sides"""
    bits = np.concatenate([np.ascontiguousarray(x, np.float32).reshape(-1), np.ascontiguousarray(y, np.float32).reshape(-1)])
    return int((bits.view(np.uint32) & np.uint32(0x7fffffff)).max()) if bits.size else 0


def peak_exp(pk):
    """pk = m 2^e with m in [0.5, 1); 0 for pk == 0"""
    return int(np.frexp(np.uint32(pk).view(np.float32))[1]) if pk else 0


def quantise(v, e):
    """clamp(rint(v 2^(13 - e)), +-8191) as int64: the product is exact, rint rounds half to even"""
    q = np.rint(np.ldexp(np.asarray(v, np.float32).astype(np.float64), QBITS - e))
    return np.clip(q, -QMAX, QMAX).astype(np.int64)


def root256(s):
    """floor(sqrt(256 s)) of an int64 array, exactly: the float64 root, corrected in integers"""
    v = np.asarray(s, np.int64) * 256
    r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    r = r - (r * r > v)
    return r + ((r + 1) * (r + 1) <= v)


def local_cost(qx, qy):
    """d [Tx][Ty] = floor(sqrt(256 sum_k (qx[i][k] - qy[j][k])^2)): |x|^2 + |y|^2 - 2 x.y, exact in int64"""
    s = (qx * qx).sum(1)[:, None] + (qy * qy).sum(1)[None, :] - 2 * (qx @ qy.T)
    return root256(s)


def allowed(Tx, Ty, r):
    """bool [Tx][Ty]: r == 0 every cell; else |i Ty - j Tx| <= r max(Tx, Ty)"""
    if r == 0:
        return np.ones((Tx, Ty), bool)
    i = np.arange(Tx, dtype=np.int64)[:, None]
    j = np.arange(Ty, dtype=np.int64)[None, :]
    return np.abs(i * Ty - j * Tx) <= np.int64(r) * max(Tx, Ty)


def recurrence(d, ok):
    """keys K [Tx][Ty] (C 2^14 + N, INF where not allowed or not reachable) and choices [Tx][Ty] (0 diagonal, 1 (i-1, j),
    2 (i, j-1)) of the cost matrix d under the mask ok, one anti-diagonal at a time"""
    Tx, Ty = d.shape
    K = np.full((Tx + 1, Ty + 1), INF, np.int64)      # K[i + 1][j + 1] = key of (i, j): row 0 and column 0 are the outside
    choice = np.zeros((Tx, Ty), np.int8)
    for s in range(Tx + Ty - 1):
        i = np.arange(max(0, s - Ty + 1), min(Tx - 1, s) + 1)
        j = s - i
        best = K[i, j].copy()                          # (i-1, j-1)
        c = np.zeros(len(i), np.int8)
        up, left = K[i, j + 1], K[i + 1, j]
        m = up < best
        best[m], c[m] = up[m], 1
        m = left < best
        best[m], c[m] = left[m], 2
        if s == 0:
            best[:] = 0
        good = ok[i, j] & (best < INF)
        K[i + 1, j + 1] = np.where(good, best + (d[i, j] << NBITS) + 1, INF)
        choice[i, j] = c
    return K[1:, 1:], choice


def backtrack(choice, n):
    Tx, Ty = choice.shape
    path = np.zeros((n, 2), np.int32)
    i, j = Tx - 1, Ty - 1
    for k in range(n - 1, -1, -1):
        path[k] = (i, j)
        c = choice[i, j]
        i, j = i - (c != 2), j - (c != 1)
    assert (i, j) in ((-1, -1), (-1, 0), (0, -1)) and tuple(path[0]) == (0, 0)
    return path


def not_defined():
    return {"total": 0, "info": np.zeros(4, np.int32), "mean": np.float32(np.nan), "path": np.zeros((0, 2), np.int32)}


def dtw(x, y, band=0, mode=WARP):
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    mode = MODES.get(mode, mode)
    Tx, Ty = len(x), len(y)
    assert x.ndim == 2 and y.ndim == 2 and x.shape[1] == y.shape[1] and 1 <= x.shape[1] <= MAX_D and max(Tx, Ty) <= MAX_FRAMES
    if Tx == 0 or Ty == 0:
        return not_defined()
    pk = peak_of(x, y)
    if pk >= 0x7f800000:
        return not_defined()
    e = peak_exp(pk)
    qx, qy = quantise(x, e), quantise(y, e)
    if mode == DIAGONAL:
        n = min(Tx, Ty)
        total = int(root256(((qx[:n] - qy[:n]) ** 2).sum(1)).sum())
        path = np.repeat(np.arange(n, dtype=np.int32)[:, None], 2, 1)
    else:
        K, choice = recurrence(local_cost(qx, qy), allowed(Tx, Ty, int(band)))
        key = int(K[-1, -1])
        if key >= int(INF):
            return not_defined()
        total, n = key >> NBITS, key & ((1 << NBITS) - 1)
        path = backtrack(choice, n)
    mean = np.float32(np.ldexp(np.float64(total) / np.float64(16 * n), e - QBITS))
    return {"total": total, "info": np.array([n, Tx, Ty, e], np.int32), "mean": mean, "path": path}
