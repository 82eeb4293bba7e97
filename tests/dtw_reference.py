"""float64 numpy restatement of dynamic time warping as include/ispk.h defines it for ispk_dtw_f32 / ispk_mcd_dtw_f32 (the
reference project has no DTW): the recurrence, the tie rule, the backtrace and the four scores.  Written from the definitions:

    D[0][0] = c[0][0];  D[i][j] = c[i][j] + min(D[i-1][j-1], D[i-1][j], D[i][j-1])
    ties go to the diagonal, then to (i-1, j), then to (i, j-1); the backtrace runs from (n-1, m-1) to (0, 0).

The table is filled one anti-diagonal at a time (its cells do not depend on each other), which is what makes 2,048 x 2,048
cells affordable in numpy; `dtw_cellwise` is the same thing cell by cell, for the hand-solved cases.
"""
import math

import numpy as np

LOGDB = 10.0 * math.sqrt(2.0) / math.log(10.0)
DIAG, UP, LEFT = 0, 1, 2          # predecessor (i-1, j-1), (i-1, j), (i, j-1)


def _backtrace(choice, n, m):
    i, j = n - 1, m - 1
    path = [(i, j)]
    while i > 0 or j > 0:
        c = choice[i, j]
        if c == DIAG:
            i, j = i - 1, j - 1
        elif c == UP:
            i -= 1
        else:
            j -= 1
        path.append((i, j))
    return np.array(path[::-1], dtype=np.int64)


def dtw_cellwise(cost):
    """(total, path int64 [K, 2]) of a float64 [n, m] cost matrix, one cell at a time."""
    cost = np.asarray(cost, dtype=np.float64)
    n, m = cost.shape
    D = np.full((n, m), np.inf)
    choice = np.zeros((n, m), dtype=np.int8)
    for i in range(n):
        for j in range(m):
            if i == 0 and j == 0:
                D[0, 0] = cost[0, 0]
                continue
            dg = D[i - 1, j - 1] if i > 0 and j > 0 else np.inf
            up = D[i - 1, j] if i > 0 else np.inf
            left = D[i, j - 1] if j > 0 else np.inf
            if dg <= up and dg <= left:
                best, c = dg, DIAG
            elif up <= left:
                best, c = up, UP
            else:
                best, c = left, LEFT
            D[i, j] = cost[i, j] + best
            choice[i, j] = c
    return float(D[n - 1, m - 1]), _backtrace(choice, n, m)


def dtw(cost):
    """(total, path int64 [K, 2]) of a float64 [n, m] cost matrix, one anti-diagonal at a time."""
    cost = np.asarray(cost, dtype=np.float64)
    n, m = cost.shape
    D = np.full((n + 1, m + 1), np.inf)             # D[i + 1, j + 1] = the table; row 0 / column 0 = the +inf border
    choice = np.zeros((n, m), dtype=np.int8)
    D[1, 1] = cost[0, 0]
    for d in range(1, n + m - 1):
        i = np.arange(max(0, d - (m - 1)), min(n - 1, d) + 1)
        j = d - i
        dg, up, left = D[i, j], D[i, j + 1], D[i + 1, j]
        is_dg = (dg <= up) & (dg <= left)
        is_up = ~is_dg & (up <= left)
        best = np.where(is_dg, dg, np.where(is_up, up, left))
        D[i + 1, j + 1] = cost[i, j] + best
        choice[i, j] = np.where(is_dg, DIAG, np.where(is_up, UP, LEFT))
    return float(D[n, m]), _backtrace(choice, n, m)


def padded_path(path, N, M):
    """int16 [N + M - 1, 2]: the path, then -1 (the layout of ispk_dtw_f32's `path`)."""
    out = np.full((N + M - 1, 2), -1, dtype=np.int16)
    out[:len(path)] = path
    return out


def is_warping_path(path, n, m):
    """From (0, 0) to (n-1, m-1) by steps (1, 1), (1, 0) and (0, 1) only."""
    path = np.asarray(path, dtype=np.int64)
    if len(path) == 0 or tuple(path[0]) != (0, 0) or tuple(path[-1]) != (n - 1, m - 1):
        return False
    step = np.diff(path, axis=0)
    ok = ((step[:, 0] == 1) & (step[:, 1] == 1)) | ((step[:, 0] == 1) & (step[:, 1] == 0)) | \
        ((step[:, 0] == 0) & (step[:, 1] == 1))
    return bool(ok.all())


def path_cost(cost, path):
    """The float64 sum of `cost` along `path`."""
    path = np.asarray(path, dtype=np.int64)
    return float(np.asarray(cost, dtype=np.float64)[path[:, 0], path[:, 1]].sum())


def cepstral_cost(mel_out, mel_target, dct):
    """float64 [n, m]: the Euclidean distance of the cepstral coefficients 1 .. n_mfcc - 1 of frame i of mel_out [C, n] and
    frame j of mel_target [C, m]; dct [C, n_mfcc]."""
    d = np.asarray(dct, dtype=np.float64)[:, 1:]
    a = np.asarray(mel_out, dtype=np.float64).T @ d
    b = np.asarray(mel_target, dtype=np.float64).T @ d
    out = np.empty((a.shape[0], b.shape[0]))
    for i in range(0, a.shape[0], 128):             # (128 rows at a time: the differences of 2,048^2 pairs do not fit at once)
        diff = a[i:i + 128, None, :] - b[None, :, :]
        out[i:i + 128] = np.sqrt((diff * diff).sum(-1))
    return out


def scores(total, path, n, m, pitch_out=None, pitch_target=None):
    """{"mcd_dtw", "f0_rmse_cents", "vuv_error", "length_ratio"} (float64) along `path`; the pitch tracks are Hz with 0 =
    unvoiced.  f0_rmse_cents is NaN when no pair of the path has both frames voiced."""
    path = np.asarray(path, dtype=np.int64)
    K = len(path)
    out = {"mcd_dtw": LOGDB * total / K, "length_ratio": n / m}
    if pitch_out is not None:
        x = np.asarray(pitch_out, dtype=np.float64)[path[:, 0]]
        y = np.asarray(pitch_target, dtype=np.float64)[path[:, 1]]
        vx, vy = x > 0, y > 0
        both = vx & vy
        if both.any():
            cents = 1200.0 * np.log2(x[both] / y[both])
            out["f0_rmse_cents"] = float(np.sqrt(np.mean(cents * cents)))
        else:
            out["f0_rmse_cents"] = float("nan")
        out["vuv_error"] = float(np.mean(vx != vy))
    return out
