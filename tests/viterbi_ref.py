"""Float64 restatement of the Viterbi decode behind ``to_viterbi_f0`` (modules/rmvpe/utils.py:26-43) and of the
f0 tail of ``RMVPE.get_pitch`` (utils/pitch_utils.py:45-51, 86-98), with the case inputs of the tests.

librosa is not needed: ``dense`` restates ``librosa.sequence.viterbi`` (0.10: ``_viterbi`` with a float64 value
table, ``log(x + tiny)`` of the probabilities, the transition and the uniform initial distribution, ``np.argmax``'s
lowest-index tie rule).  This restatement, not librosa itself, is the oracle of the native kernel.
"""
import numpy as np

N_CLASS, WIDTH = 360, 30
TINY = float(np.finfo(np.float32).tiny)


def transition(n=N_CLASS, w=WIDTH):
    xx, yy = np.meshgrid(range(n), range(n))
    A = np.maximum(w - abs(xx - yy), 0)
    return A / A.sum(axis=1, keepdims=True)


def log_prob(hidden):
    """hidden [T, n] -> lp [T, n], normalised in float64 (the native rule)."""
    h = np.asarray(hidden, np.float64)
    return np.log(h / h.sum(axis=1, keepdims=True) + TINY)


def log_prob_f32norm(hidden):
    """The reference's own arithmetic: the float32 salience normalised in float32, then librosa's float64 log."""
    prob = np.asarray(hidden, np.float32).T
    prob = prob / prob.sum(axis=0)
    return np.log(prob.T + np.finfo(np.float32).tiny).astype(np.float64)


def recurse_dense(lp, n, w):
    """-> (val [T, n], path [T]) by the full n x n maximisation."""
    T = lp.shape[0]
    lt = np.log(transition(n, w) + TINY)
    val = np.zeros((T, n))
    ptr = np.zeros((T, n), np.int64)
    val[0] = lp[0] + np.log(1.0 / n + TINY)
    for t in range(1, T):
        tr = val[t - 1][:, None] + lt                  # [i, j]
        ptr[t] = np.argmax(tr, axis=0)
        val[t] = lp[t] + tr[ptr[t], np.arange(n)]
    return val, backtrace(val, ptr)


def backtrace(val, ptr):
    T = val.shape[0]
    path = np.zeros(T, np.int64)
    path[-1] = np.argmax(val[-1])
    for t in range(T - 2, -1, -1):
        path[t] = ptr[t + 1, path[t + 1]]
    return path


def dense(hidden, w=WIDTH):
    return recurse_dense(log_prob(hidden), np.shape(hidden)[1], w)


def dense_f32norm(hidden, w=WIDTH):
    return recurse_dense(log_prob_f32norm(hidden), np.shape(hidden)[1], w)


def banded(hidden, w=WIDTH, lp=None):
    """The reduced form the kernel evaluates: the 2 w - 1 in-band predecessors plus the lowest global argmax of
    val[t - 1] where that lies outside the state's band."""
    lp = log_prob(hidden) if lp is None else lp
    T, n = lp.shape
    lt = np.log(transition(n, w) + TINY)
    log_off = np.log(0.0 + TINY)
    val = np.zeros((T, n))
    ptr = np.zeros((T, n), np.int64)
    val[0] = lp[0] + np.log(1.0 / n + TINY)
    for t in range(1, T):
        prev = val[t - 1]
        g = int(np.argmax(prev))
        for j in range(n):
            lo, hi = max(j - w + 1, 0), min(j + w, n)
            cand = prev[lo:hi] + lt[lo:hi, j]
            k = int(np.argmax(cand))
            best, arg = cand[k], lo + k
            if abs(g - j) >= w:
                c = prev[g] + log_off
                if c > best or (c == best and g < arg):
                    best, arg = c, g
            ptr[t, j] = arg
            val[t, j] = lp[t, j] + best
    return val, backtrace(val, ptr)


def dense_from_lp(lp, w=WIDTH):
    return recurse_dense(lp, lp.shape[1], w)


# ---------------------------------------------------------------- case inputs
def ridge(T, n, centre, sigma=1.5, floor=1e-4, seed=0):
    rng = np.random.default_rng(seed)
    j = np.arange(n)[None, :]
    c = np.asarray(centre, np.float64).reshape(T, 1)
    return (np.exp(-0.5 * ((j - c) / sigma) ** 2) + floor * rng.random((T, n))).astype(np.float32)


def case(name, T, n=N_CLASS, seed=0):
    """float32 [T, n] salience (values >= 0)."""
    t = np.arange(T)
    if name == "rand":
        return np.random.default_rng(seed).random((T, n)).astype(np.float32)
    if name == "glide":
        return ridge(T, n, (100 + 40 * np.sin(t / 9.0)) * n / N_CLASS, seed=seed)
    if name in ("jump", "zeros"):
        h = ridge(T, n, np.where(t < T // 2, 50, 300) * n / N_CLASS, seed=seed)
        if name == "zeros":
            h[:, :20 * n // N_CLASS] = 0.0
            if T > 2:
                one = T // 3
                keep = h[one].argmax()
                v = h[one, keep]
                h[one] = 0.0
                h[one, keep] = v
        return h
    if name == "uniform":
        return np.full((T, n), 0.25, np.float32)
    raise KeyError(name)


CASE_NAMES = ("rand", "glide", "jump", "zeros", "uniform")


# ---------------------------------------------------------------- the f0 tail
def interp_f0(f0):
    """utils/pitch_utils.py:45-51 on a float32 curve -> (f0 float32, uv)."""
    f0 = np.asarray(f0, np.float32)
    uv = f0 == 0
    with np.errstate(divide="ignore"):
        lf = np.log2(f0 + uv)
    lf[uv] = -np.inf
    if uv.any() and not uv.all():
        lf[uv] = np.interp(np.where(uv)[0], np.where(~uv)[0], lf[~uv])
    return 2 ** lf, uv


def resample_align_curve(points, t_src, t_dst, length):
    """utils/pitch_utils.py:86-98."""
    t_max = (len(points) - 1) * t_src
    curve = np.interp(np.arange(0, t_max, t_dst), t_src * np.arange(len(points)), points).astype(points.dtype)
    if len(curve) > length:
        return curve[:length]
    if len(curve) < length:
        return np.concatenate((curve, np.full(length - len(curve), curve[-1], dtype=curve.dtype)))
    return curve


def uv_curve(f0, t_src, t_dst, length):
    """The interpolated unvoiced flags before the 0.5 threshold, float64 (for the distance-from-0.5 check)."""
    uv = (np.asarray(f0) == 0).astype(np.float64)
    return resample_align_curve(uv, t_src, t_dst, length)


def align_f0(f0, t_src, t_dst, length, interp_uv=False):
    """component/pe/rmvpe.py:57-72 after infer_from_audio -> (f0 float32 [length], uv bool [length])."""
    f, uv = interp_f0(f0)
    f_res = resample_align_curve(f, t_src, t_dst, length)
    uv_res = resample_align_curve(uv.astype(np.float32), t_src, t_dst, length) > 0.5
    if not interp_uv:
        f_res[uv_res] = 0
    return f_res, uv_res


def f0_rows(n, seed=0):
    """{name: float32 [n]}: unvoiced runs at the head, in the middle and at the tail, all voiced, all unvoiced,
    a single voiced frame."""
    rng = np.random.default_rng(seed + n)
    base = (110.0 * 2 ** (rng.random(n) * 2.5)).astype(np.float32)
    rows = {"voiced": base.copy(), "unvoiced": np.zeros(n, np.float32)}
    runs = base.copy()
    if n >= 8:
        runs[:n // 7 + 1] = 0
        runs[n // 3:n // 3 + n // 5 + 1] = 0
        runs[n // 2 + n // 4::2] = 0
        runs[-(n // 9 + 1):] = 0
    else:
        runs[0] = 0
    rows["runs"] = runs
    single = np.zeros(n, np.float32)
    single[n // 2] = base[n // 2]
    rows["single"] = single
    mid = base.copy()
    mid[1:-1] = 0 if n > 2 else mid[1:-1]
    rows["ends"] = mid
    return rows


# (t_src, t_dst): the network's 10 ms grid onto hop / samplerate grids whose frames never fall on a source
# midpoint, and one pair that stretches the curve
GRIDS = ((0.01, 512 / 44100), (0.01, 128 / 24000), (0.01, 256 / 44100))
