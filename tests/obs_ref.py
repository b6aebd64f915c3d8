"""The 44 trace-only entries of the 53-float observation, evaluated in plain NumPy from the observation's definition.

Test infrastructure: nothing in dc_rl_amd/ imports it, and it shares no text with the device's closed forms and reduction trees
(csrc/sdc_features.hip slope_of / np_sum, csrc/sdc_device.hpp build_obs_pool) nor with the oracle's C.  Every number comes out of
NumPy's own routine for the operation the definition names:

  sustaindc_env.py:313-314   np.convolve(..., ones(4), 'valid') / 4 over [cur, futures] and over [pasts, cur]
  sustaindc_env.py:317-318   np.polyfit(range(n), smoothed, 1)[0]
  sustaindc_env.py:331       np.polyfit over [cur temperature, 16 futures], no smoothing
  sustaindc_env.py:266-300   np.mean, np.std, np.gradient(hstack(cur, values)), the first sign change of the gradient, and
                             (cur - mean) / (std + 1e-8)
  sustaindc_env.py:342, 386-393, 426-432   which entries each agent's state holds, and the fp32 cast
  utils/managers.py:79-84    the hour's cos / sin of round(hour / 24, 3) * 2 pi, scaled into [0, 1]
  utils/managers.py:437, 608 the normalised traces (the caller hands them in)
  utils/managers.py:482-483  the past slice norm_carbon[i' - 16 : i'], which is EMPTY while i' < 16

Held to the reference's recorded float32 observations bit for bit by tests/test_obs_ref.py, and the device to it by
tests/test_gpu_obs_features.py.
"""
import numpy as np

N_FUTURE_CI = 8      # carbon-intensity forecast entries after the current one
N_FUTURE_T = 16      # temperature forecast entries
N_PAST_CI = 16       # past carbon-intensity entries (utils/managers.py:482-483)

# raw-observation layout (tests/gpu_helpers.raw_obs): ls 26 | dc 14 | bat 13
LS, DC, BAT = 0, 26, 40
SHARED10 = ("cos", "sin", "nc", "ci_future_slope", "ci_past_slope", "ci_mean", "ci_std", "ci_pct", "ci_peak", "ci_valley")
T6 = ("t_slope", "t_mean", "t_std", "t_pct", "t_peak", "t_valley")
INDEX = {}           # raw-obs index -> the name of the quantity it holds
for _a in (LS, DC, BAT):
    INDEX.update({_a + k: name for k, name in enumerate(SHARED10)})
INDEX.update({LS + 13: "w", LS + 14: "nt"})
INDEX.update({LS + 15 + k: name for k, name in enumerate(T6)})
INDEX.update({DC + 10: "w", DC + 11: "w_next", DC + 12: "nt", DC + 13: "nt_next"})
INDEX.update({BAT + 10: "w", BAT + 11: "nt"})
assert len(INDEX) == 44
SLOPES = ("ci_future_slope", "ci_past_slope", "t_slope")
SLOPE_INDEX = sorted(i for i, name in INDEX.items() if name in SLOPES)
EXACT_INDEX = sorted(i for i, name in INDEX.items() if name not in SLOPES)

# The slope bound |device - np.polyfit| <= 2^-24 |ref| + SLOPE_C 2^-53 max|y|: the first term is the device's fp32 cast, the second
# np.polyfit's own distance from the exact least-squares slope (an SVD solve, against the device's closed form).  SLOPE_C is 4 x the
# worst |np.polyfit - longdouble closed form| / (2^-53 max|y|) over every slope window of every constructed case of tests/obs_cases.py,
# rounded up; the 4 covers the device's different but equally valid summation order.  Measured worst: 2.31, on the four equal points
# of an empty past (tests/test_obs_ref.py re-measures it and fails if this constant is below 4 x the measurement).
SLOPE_C = 10
SLOPE_SAFETY = 4


def window_features(values, cur):
    """mean, std, (cur - mean) / (std + 1e-8), time to the next peak / n, time to the next valley / n of `values` following `cur`
    (sustaindc_env.py:266-300) -> (the five numbers, the gradient they were read from)"""
    values = np.asarray(values, dtype=np.float64)
    n = len(values)
    mean, std = np.mean(values), np.std(values)
    g = np.gradient(np.hstack((cur, values)))
    peaks = np.nonzero((g[:-1] > 0) & (g[1:] <= 0))[0]
    valleys = np.nonzero((g[:-1] < 0) & (g[1:] >= 0))[0]
    peak = peaks[0] if len(peaks) else n
    valley = valleys[0] if len(valleys) else n
    return [mean, std, (cur - mean) / (std + 1e-8), peak / n, valley / n], g


def slope_windows(NC, NT, win_lo, ip):
    """the three windows np.polyfit sees at table cursor `ip`: smoothed CI future (6 points), smoothed CI past (14 points, or 4 while
    there is no past), temperature (17 points).  NC / NT[k] hold the normalised traces at table index win_lo + k."""
    k = ip - win_lo
    cur = NC[k]
    future = NC[k + 1:k + 1 + N_FUTURE_CI]
    past = NC[k - N_PAST_CI:k] if ip >= N_PAST_CI else NC[0:0]
    box = np.ones(4)
    return (np.convolve(np.hstack((cur, future)), box, "valid") / 4, np.convolve(np.hstack((past, cur)), box, "valid") / 4,
            np.hstack((NT[k], NT[k + 1:k + 1 + N_FUTURE_T])))


def polyfit_slope(y):
    return np.polyfit(range(len(y)), y, 1)[0]


def slope_longdouble(y):
    """the least-squares slope of y over 0 .. n-1 in closed form, in np.longdouble: only to SIZE the slope bound (SLOPE_C), never
    compared with the device"""
    y = np.asarray(y, dtype=np.longdouble)
    x = np.arange(len(y), dtype=np.longdouble)
    dx = x - x.sum() / len(y)
    return (dx * (y - y.sum() / len(y))).sum() / (dx * dx).sum()


def slope_scale(y):
    """what the slope bound is relative to: the largest |y| of the window"""
    return float(np.max(np.abs(y)))


def hour_features(hour):
    """utils/managers.py:79-84: Python's round on a Python float, as the reference's time manager holds the hour"""
    angle = round(float(hour) / 24, 3) * (np.pi * 2)
    return np.cos(angle) * 0.5 + 0.5, np.sin(angle) * 0.5 + 0.5


def trace_quantities(NC, NT, W, win_lo, ip, hour):
    """{name: fp64 value} of the trace-only quantities at table cursor `ip` and hour of day `hour`, plus "_y": the three slope
    windows and "_g": the two gradients (for the slope bound and the censuses of tests/obs_cases.py)"""
    k = ip - win_lo
    ys = slope_windows(NC, NT, win_lo, ip)
    ci5, g_ci = window_features(NC[k + 1:k + 1 + N_FUTURE_CI], NC[k])
    t5, g_t = window_features(NT[k + 1:k + 1 + N_FUTURE_T], NT[k])
    cos_h, sin_h = hour_features(hour)
    q = dict(cos=cos_h, sin=sin_h, nc=NC[k], w=W[k], w_next=W[k + 1], nt=NT[k], nt_next=NT[k + 1])
    q.update(zip(SLOPES, (polyfit_slope(y) for y in ys)))
    q.update(zip(("ci_mean", "ci_std", "ci_pct", "ci_peak", "ci_valley"), ci5))
    q.update(zip(("t_mean", "t_std", "t_pct", "t_peak", "t_valley"), t5))
    q["_y"] = dict(zip(SLOPES, ys))
    q["_g"] = dict(ci=g_ci, t=g_t)
    return q


def trace_obs(NC, NT, W, win_lo, ip, hour):
    """{raw-obs index: fp64 value} for the 44 trace-only entries of the observation taken at table cursor `ip` (= i') and hour of
    day `hour`; NC, NT, W[k] hold the normalised carbon intensity, the normalised temperature and the workload at table index
    win_lo + k"""
    q = trace_quantities(NC, NT, W, win_lo, ip, hour)
    return {i: float(q[name]) for i, name in INDEX.items()}


def hour_at(init_hour, s):
    """the time manager's hour `s` quarter-hour steps after a start at the whole hour `init_hour` (utils/managers.py:135-138)"""
    return ((int(init_hour) * 4 + s) % 96) / 4


def episode_table(NC, NT, W, win_lo, c0, init_hour, rows):
    """trace_obs for the observations at cursors c0 + s, s in `rows` -> (values [len(rows), 44] fp64 in the order of sorted(INDEX),
    slope scales [len(rows), 3]: max|y| of the three slope windows)"""
    cols = sorted(INDEX)
    out = np.zeros((len(rows), len(cols)))
    scale = np.zeros((len(rows), 3))
    for r, s in enumerate(rows):
        q = trace_quantities(NC, NT, W, win_lo, c0 + s, hour_at(init_hour, s))
        out[r] = [q[INDEX[i]] for i in cols]
        scale[r] = [slope_scale(q["_y"][name]) for name in SLOPES]
    return out, scale
