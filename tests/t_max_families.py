"""The families of t_max an occlusion query is tried with, shared by tests/ray_query_driver.py, tests/any_hit_driver.py and
tests/any_hit_rays.py.  Not a test module; it needs numpy alone."""
import numpy as np

T_MAX_OF_HITS = ("below", "equal", "above", "half", "double", "zero", "minus one", "inf", "nan")
T_MAX_OF_MISSES = ("one", "inf", "nan")


def t_max_for(sc):
    """Every family of t_max, dealt round-robin among the hits and among the misses of sc (its t and idx, idx < 0 a miss) ->
    (t_max, the specification's answer, family of every ray)"""
    t, hit = sc.t, sc.idx >= 0
    n = len(t)
    t_max = np.zeros(n, np.float32)
    family = np.empty(n, object)
    inf, zero = np.float32(np.inf), np.float32(0.0)
    of_hit = {"below": np.nextafter(t, zero), "equal": t, "above": np.nextafter(t, inf), "half": np.float32(0.5) * t, "double": np.float32(2.0) * t,
              "zero": np.zeros_like(t), "minus one": np.full_like(t, -1.0), "inf": np.full_like(t, np.inf), "nan": np.full_like(t, np.nan)}
    of_miss = {"one": np.ones_like(t), "inf": np.full_like(t, np.inf), "nan": np.full_like(t, np.nan)}
    for rows, table, names in ((np.flatnonzero(hit), of_hit, T_MAX_OF_HITS), (np.flatnonzero(~hit), of_miss, T_MAX_OF_MISSES)):
        for k, name in enumerate(names):
            mine = rows[k::len(names)]
            t_max[mine] = table[name][mine]
            family[mine] = name
    with np.errstate(invalid="ignore"):
        want = (hit & (t < t_max)).astype(np.int32)                      # one f32 compare against the closest hit
    return t_max, want, family
