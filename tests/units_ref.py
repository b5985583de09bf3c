"""include/swc_units.h restated in plain Python / numpy, from the header's text alone: plain loops for the histogram, the
repeats and the positional counts, the textbook two-row Levenshtein recurrence, dedup as a loop.  The tests compare the
kernels with this bit for bit.  Rows are [G][T] integer arrays (numpy or nested lists)."""
import numpy as np

MAX_GROUPS, MAX_CODES, MAX_FRAMES, CHUNK, STRIP = 8, 16384, 8192, 1024, 256
USAGE_MAX_FRAMES = 1 << 24


def n_codes_of(levels):
    n = 1
    for v in levels:
        n *= int(v)
    return n


def valid(v, n_codes):
    return 0 <= int(v) < n_codes


def equal(x, y, n_codes):
    """both valid and the same number: an invalid value equals nothing, itself included"""
    return valid(x, n_codes) and valid(y, n_codes) and int(x) == int(y)


def code_levels(c, levels):
    """level d = (c / base_d) % L_d with base = 1, L0, L0 L1, L0 L1 L2"""
    out, c = [], int(c)
    for L in levels:
        out.append(c % int(L))
        c //= int(L)
    return out


def clamp(T, max_frames):
    return 0 if T < 0 else (max_frames if T > max_frames else int(T))


def usage(rows_list, levels, G, max_frames=None, hist=None, repeats=None, totals=None):
    """swc_code_usage: adds into (hist int64 [G][n_codes], repeats int64 [G], totals int64 [2]) and returns them"""
    n_codes = n_codes_of(levels)
    hist = np.zeros((G, n_codes), dtype=np.int64) if hist is None else hist
    repeats = np.zeros(G, dtype=np.int64) if repeats is None else repeats
    totals = np.zeros(2, dtype=np.int64) if totals is None else totals
    for rows in rows_list:
        rows = np.asarray(rows)
        T = rows.shape[1]
        T = T if max_frames is None else clamp(T, max_frames)
        totals[0] += T
        for g in range(G):
            for t in range(T):
                v = int(rows[g][t])
                if valid(v, n_codes):
                    hist[g][v] += 1
                else:
                    totals[1] += 1
                if t >= 1 and equal(v, rows[g][t - 1], n_codes):
                    repeats[g] += 1
    return hist, repeats, totals


def dedup(seq, n_codes):
    """value t is kept when t == 0 or it does not equal value t - 1"""
    out = []
    for t, v in enumerate(seq):
        if t == 0 or not equal(v, seq[t - 1], n_codes):
            out.append(int(v))
    return out


def levenshtein(a, b, n_codes):
    """unit costs; two symbols match when `equal`.  The two-row recurrence.  (Invalid values become -1 on one side and -2 on the
    other first, so that the inner loop's plain == is `equal`.)"""
    a = [int(x) if valid(x, n_codes) else -1 for x in a]
    b = [int(y) if valid(y, n_codes) else -2 for y in b]
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        x = a[i - 1]
        for j in range(1, len(b) + 1):
            sub = prev[j - 1] + (0 if x == b[j - 1] else 1)
            cur[j] = min(sub, prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


def compare(rows_a, rows_b, levels, G, do_dedup=True, max_frames=MAX_FRAMES):
    """swc_code_compare for ONE pair -> dict of int32 arrays without the leading B: match, both_valid, edit, len_a, len_b [G];
    level_match, level_l1 [G][4]; frame_match (); bad [2]"""
    n_codes = n_codes_of(levels)
    rows_a, rows_b = np.asarray(rows_a), np.asarray(rows_b)
    Ta, Tb = clamp(rows_a.shape[1], max_frames), clamp(rows_b.shape[1], max_frames)
    n = min(Ta, Tb)
    r = {k: np.zeros(G, dtype=np.int32) for k in ("match", "both_valid", "edit", "len_a", "len_b")}
    r["level_match"], r["level_l1"] = np.zeros((G, 4), dtype=np.int32), np.zeros((G, 4), dtype=np.int32)
    r["bad"] = np.zeros(2, dtype=np.int32)
    frame = 0
    for t in range(n):
        all_equal = True
        for g in range(G):
            x, y = int(rows_a[g][t]), int(rows_b[g][t])
            if equal(x, y, n_codes):
                r["match"][g] += 1
            else:
                all_equal = False
            if valid(x, n_codes) and valid(y, n_codes):
                r["both_valid"][g] += 1
                for d, (p, q) in enumerate(zip(code_levels(x, levels), code_levels(y, levels))):
                    r["level_match"][g][d] += p == q
                    r["level_l1"][g][d] += abs(p - q)
        frame += all_equal
    r["frame_match"] = np.int32(frame)
    for g in range(G):
        r["bad"][0] += sum(not valid(v, n_codes) for v in rows_a[g][:Ta])
        r["bad"][1] += sum(not valid(v, n_codes) for v in rows_b[g][:Tb])
        a, b = [int(v) for v in rows_a[g][:Ta]], [int(v) for v in rows_b[g][:Tb]]
        if do_dedup:
            a, b = dedup(a, n_codes), dedup(b, n_codes)
        r["len_a"][g], r["len_b"][g] = len(a), len(b)
        r["edit"][g] = levenshtein(a, b, n_codes)
    return r


def compare_batch(list_a, list_b, levels, G, do_dedup=True, max_frames=MAX_FRAMES):
    """-> the dict of compare() with the leading B"""
    per = [compare(a, b, levels, G, do_dedup, max_frames) for a, b in zip(list_a, list_b)]
    return {k: np.stack([p[k] for p in per]).astype(np.int32) for k in per[0]}
