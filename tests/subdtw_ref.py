"""swc_cmvn and swc_subdtw of include/swc_subdtw.h restated in numpy (float64 and int64), written from the header's text: THE
reference of tests/test_subdtw_cpu.py and tests/test_subdtw_gpu.py (and the host yardstick of tools/bench_warpq.py).  Nothing
here imports the package.

    out = cmvn(c)                                     c f32 [T][K] -> f32 [T][K]
    r = subdtw(q, y, Lp, Sp, steps)                   q f32 [Tq][D], y f32 [Ty][D]
    r["cost"] int64 [P], r["info"] int32 [P][4] = N, start, end, status, r["score"] float64, r["patches"] = (ok, P), r["e"]

brute(d, steps) is an independent statement of one patch: the enumeration of every step sequence, for tiny cases.
"""
import numpy as np

MAX_PATCH, MAX_STEPS, MAX_STRIDE, MAX_FRAMES, MAX_D, QBITS, NBITS = 256, 4, 3, 8192, 32, 13, 14
QMAX = (1 << QBITS) - 1
ST_OK, ST_UNREACHABLE, ST_UNDEFINED, ST_QUERY = 0, 1, 2, 3
CMVN_BLOCK = 256
INF = np.int64(1) << np.int64(62)
D_MAX = 91 * 2 * QMAX
SYMMETRIC = ((1, 1), (1, 0), (0, 1))
WARPQ = ((1, 1), (3, 2), (1, 3))          # metrics.warpq's default
ASYMMETRIC = ((1, 0), (0, 3), (1, 3))     # no step walks the diagonal: an identical pair does not score 0 under it


# ---- swc_cmvn ----

def block_sum(v):
    """S(v) of the header for every column of v float64 [T][K]: blocks of 256 frames serially in ascending t from 0.0, then the
    blocks' sums serially in ascending block order from 0.0 (vectorised over the blocks and the columns: the order of every
    column's additions is the stated one)"""
    T, K = v.shape
    nblk = -(-T // CMVN_BLOCK)
    pad = np.zeros((nblk * CMVN_BLOCK, K), np.float64)
    pad[:T] = v
    pad = pad.reshape(nblk, CMVN_BLOCK, K)
    live = (np.arange(nblk * CMVN_BLOCK) < T).reshape(nblk, CMVN_BLOCK)
    part = np.zeros((nblk, K), np.float64)
    for t in range(CMVN_BLOCK):
        part = np.where(live[:, t, None], part + pad[:, t], part)
    total = np.zeros(K, np.float64)
    for b in range(nblk):
        total = total + part[b]
    return total


def cmvn(c):
    c = np.asarray(c, np.float32)
    T, K = c.shape
    if T == 0:
        return c.copy()
    v = c.astype(np.float64)
    with np.errstate(all="ignore"):
        m = block_sum(v) / np.float64(T)
        d = v - m[None, :]
        var = block_sum(d * d) / np.float64(T)
        out = (d / np.sqrt(var)[None, :]).astype(np.float32)
    out[:, var == 0.0] = 0.0
    return out


# ---- swc_subdtw ----

def peak_of(x, y):
    bits = np.concatenate([np.ascontiguousarray(x, np.float32).reshape(-1), np.ascontiguousarray(y, np.float32).reshape(-1)])
    return int((bits.view(np.uint32) & np.uint32(0x7fffffff)).max()) if bits.size else 0


def peak_exp(pk):
    return int(np.frexp(np.uint32(pk).view(np.float32))[1]) if pk else 0


def quantise(v, e):
    q = np.rint(np.ldexp(np.asarray(v, np.float32).astype(np.float64), QBITS - e))
    return np.clip(q, -QMAX, QMAX).astype(np.int64)


def root256(s):
    v = np.asarray(s, np.int64) * 256
    r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    r = r - (r * r > v)
    return r + ((r + 1) * (r + 1) <= v)


def local_cost(qx, qy):
    s = (qx * qx).sum(1)[:, None] + (qy * qy).sum(1)[None, :] - 2 * (qx @ qy.T)
    return root256(s)


def patch_count(Tq, Lp, Sp):
    if Lp == 0:
        return 1 if 1 <= Tq <= MAX_PATCH else 0
    return 0 if Tq < Lp else 1 + (Tq - Lp) // Sp


def check_steps(steps):
    st = [(int(a), int(b)) for a, b in steps]
    assert 1 <= len(st) <= MAX_STEPS and len(set(st)) == len(st) and any(a >= 1 for a, _ in st)
    assert all(0 <= a <= MAX_STRIDE and 0 <= b <= MAX_STRIDE and a + b >= 1 for a, b in st)
    return st


def patch_dp(d, steps):
    """one patch: d int64 [L][Ty] -> (cost, N, start, end, status); row by row, every row vectorised over j.  A row's cells
    depend on earlier rows and, through the steps with di == 0, on earlier cells of the same row: those are taken column by
    column"""
    L, Ty = d.shape
    if Ty == 0:
        return 0, 0, 0, 0, ST_UNREACHABLE
    key = np.full((L, Ty), INF, np.int64)
    org = np.zeros((L, Ty), np.int64)
    key[0] = (d[0] << NBITS) + 1
    org[0] = np.arange(Ty)
    up = [(k, di, dj) for k, (di, dj) in enumerate(steps) if di >= 1]
    same = [(k, dj) for k, (di, dj) in enumerate(steps) if di == 0]
    for i in range(1, L):
        best = np.full(Ty, INF, np.int64)
        who = np.full(Ty, len(steps), np.int64)      # the step that gave best (ties: the smaller index)
        bo = np.zeros(Ty, np.int64)
        for k, di, dj in up:
            if i - di < 0 or dj >= Ty:
                continue
            cand = np.full(Ty, INF, np.int64)
            cand[dj:] = key[i - di, :Ty - dj]
            co = np.zeros(Ty, np.int64)
            co[dj:] = org[i - di, :Ty - dj]
            m = (cand < best) | ((cand == best) & (cand < INF) & (k < who))
            best[m], who[m], bo[m] = cand[m], k, co[m]
        if not same:
            ok = best < INF
            key[i] = np.where(ok, best + (d[i] << NBITS) + 1, INF)
            org[i] = bo
            continue
        for j in range(Ty):
            b, w, o = best[j], who[j], bo[j]
            for k, dj in same:
                if j - dj >= 0:
                    c = key[i, j - dj]
                    if c < b or (c == b and c < INF and k < w):
                        b, w, o = c, k, org[i, j - dj]
            if b < INF:
                key[i, j] = b + (d[i, j] << NBITS) + 1
                org[i, j] = o
    last = key[L - 1]
    j = int(np.argmin(last))                         # the first of equal minima: the smallest j
    if last[j] >= INF:
        return 0, 0, 0, 0, ST_UNREACHABLE
    k = int(last[j])
    return k >> NBITS, k & ((1 << NBITS) - 1), int(org[L - 1, j]), j, ST_OK


def median_score(costs, e):
    """the median of a list of exact integer costs, scaled once by 2^(e - 13) / 16 in float64; NaN for an empty list"""
    n = len(costs)
    if n == 0:
        return np.float64(np.nan)
    s = sorted(int(c) for c in costs)
    lo, hi = s[(n - 1) // 2], s[n // 2]
    return np.ldexp(np.float64(lo + hi) * np.float64(0.5), e - QBITS - 4)


def subdtw(q, y, Lp, Sp, steps):
    q, y = np.asarray(q, np.float32), np.asarray(y, np.float32)
    steps = check_steps(steps)
    Tq, Ty = len(q), len(y)
    assert q.ndim == 2 and y.ndim == 2 and q.shape[1] == y.shape[1] and 1 <= q.shape[1] <= MAX_D and max(Tq, Ty) <= MAX_FRAMES
    assert 0 <= Lp <= MAX_PATCH and Sp >= 1
    P = patch_count(Tq, Lp, Sp)
    cost = np.zeros(P, np.int64)
    info = np.zeros((P, 4), np.int32)
    res = {"cost": cost, "info": info, "e": 0, "query_status": ST_QUERY if (Lp == 0 and P == 0) else None}
    defined = False
    if Tq > 0 and Ty > 0:                               # an empty pair's features are not read
        pk = peak_of(q, y)
        defined = pk < 0x7f800000
        if defined:
            res["e"] = peak_exp(pk)
            qq, qy = quantise(q, res["e"]), quantise(y, res["e"])
    L = Lp if Lp > 0 else Tq
    for p in range(P):
        if Ty == 0:
            info[p, 3] = ST_UNREACHABLE
        elif not defined:
            info[p, 3] = ST_UNDEFINED
        else:
            i0 = p * Sp if Lp > 0 else 0
            c, n, a, b, st = patch_dp(local_cost(qq[i0:i0 + L], qy), steps)
            cost[p], info[p] = c, (n, a, b, st)
    ok = info[:, 3] == ST_OK
    res["score"] = median_score(cost[ok], res["e"])
    res["patches"] = (int(ok.sum()), P)
    return res


def brute(d, steps):
    """(key, start, end) of one patch by enumerating every step sequence from every start (0, j0): the smallest key C 2^14 + N
    over all paths that end in row L - 1; among paths of one key that end in one cell, the header's recurrence keeps the one whose
    LAST step comes first in `steps`, then (recursively) the one that was kept for the predecessor.  That is a lexicographic
    order on the reversed sequence of step indices, which is what is compared here.  None when no path reaches row L - 1."""
    L, Ty = d.shape
    best = None
    stack = [(0, j0, int(d[0, j0]), 1, j0, ()) for j0 in range(Ty)]
    while stack:
        i, j, c, n, j0, rev = stack.pop()
        if i == L - 1:
            cand = ((c << NBITS) + n, j, rev, j0)
            if best is None or cand[:3] < best[:3]:
                best = cand
        for k, (di, dj) in enumerate(steps):
            ii, jj = i + di, j + dj
            if ii < L and jj < Ty:
                stack.append((ii, jj, c + int(d[ii, jj]), n + 1, j0, (k,) + rev))
    if best is None:
        return None
    return best[0], best[3], best[1]
