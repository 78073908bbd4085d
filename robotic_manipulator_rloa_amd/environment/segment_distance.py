"""Distances between the segments that carry the arm's capsules and a point, another segment or a box: the closed forms
KinematicEnvironment (environment/kinematic.py) evaluates in float64 and csrc/chain_env.hip in float32. Pure functions of arrays of
points [..., 3], which broadcast."""
import numpy as np


def segment_point_distance2(a: np.ndarray, b: np.ndarray, c: np.ndarray):
    """Squared distance from point c to the segment a-b (projection clamped to [0, 1]); arrays of points [..., 3] broadcast."""
    ab, ac = b - a, c - a
    den = np.sum(ab * ab, axis=-1)
    t = np.clip(np.sum(ac * ab, axis=-1) / np.where(den > 0.0, den, 1.0), 0.0, 1.0)
    d = ac - t[..., None] * ab
    return np.sum(d * d, axis=-1)


def segment_segment_distance2(a1: np.ndarray, b1: np.ndarray, a2: np.ndarray, b2: np.ndarray):
    """Squared distance between the segments a1-b1 and a2-b2; arrays of points [..., 3] broadcast.
    The minimum over five candidates, each the squared distance between two points that DO lie on the two segments, so none is
    below the answer: the four end-point-to-segment distances, and the closest points of the two carrying lines (closed form,
    clamped into the segments, then each parameter projected once more given the other). One of them attains it: the minimum
    over the square [0, 1]^2 of the two parameters is either interior — then it is the lines' closest pair — or has a parameter
    at 0 or 1, an end point against the other segment. The closed form's denominator |u|^2 |v|^2 - (u.v)^2 vanishes for parallel
    or zero-length segments; it is guarded and the candidate then starts from parameter 0, which loses nothing: between parallel
    segments the minimum is also attained at an end point, and a zero-length segment is an end point."""
    u, v, w = b1 - a1, b2 - a2, a1 - a2
    a, b, c = np.sum(u * u, axis=-1), np.sum(u * v, axis=-1), np.sum(v * v, axis=-1)
    d, e = np.sum(u * w, axis=-1), np.sum(v * w, axis=-1)
    den = a * c - b * b
    ok = den > 1e-14 * a * c
    s = np.clip(np.where(ok, (b * e - c * d) / np.where(ok, den, 1.0), 0.0), 0.0, 1.0)
    t = np.clip((b * s + e) / np.where(c > 0.0, c, 1.0), 0.0, 1.0) * (c > 0.0)
    s = np.clip((b * t - d) / np.where(a > 0.0, a, 1.0), 0.0, 1.0) * (a > 0.0)
    x = w + s[..., None] * u - t[..., None] * v
    best = np.sum(x * x, axis=-1)
    for cand in (segment_point_distance2(a2, b2, a1), segment_point_distance2(a2, b2, b1),
                 segment_point_distance2(a1, b1, a2), segment_point_distance2(a1, b1, b2)):
        best = np.minimum(best, cand)
    return best


def segment_box_distance(a: np.ndarray, b: np.ndarray, half: np.ndarray):
    """Distance between the segment a-b and the box |x_i| <= half_i, the points given in the box's frame; arrays [..., 3]
    broadcast. 0 for a segment that touches or enters the box: the rule reports no penetration depth.
    With p(t) = a + t (b - a), f(t) = sum_i max(|p_i(t)| - half_i, 0)^2 is convex, C1 and piecewise quadratic: f' is non-decreasing
    and linear between its knots — 0, 1 and the up to six t in (0, 1) at which a coordinate crosses a face plane, p_i(t) = +-half_i.
    Sorted, the knots bracket the root of f': the last one with f' <= 0 and the first with f' >= 0, between which f' is linear. f' > 0
    at 0 puts the minimum at t = 0, f' < 0 at 1 at t = 1; a zero-length segment has f' = 0 throughout and takes t = 0."""
    a, b, half = np.broadcast_arrays(np.asarray(a, float), np.asarray(b, float), np.asarray(half, float))
    u = b - a

    def slope(t):                                         # f'(t) / 2
        x = a + t[..., None] * u
        return np.sum((x - np.clip(x, -half, half)) * u, axis=-1)

    with np.errstate(divide="ignore", invalid="ignore"):
        knots = np.concatenate([(half - a) / u, (-half - a) / u], axis=-1)
    knots = np.where(np.isfinite(knots), np.clip(knots, 0.0, 1.0), 0.0)       # (an axis the segment does not move along: no knot)
    lead = knots.shape[:-1]
    knots = np.sort(np.concatenate([np.zeros(lead + (1,)), knots, np.ones(lead + (1,))], axis=-1), axis=-1)
    g = np.stack([slope(knots[..., k]) for k in range(8)], axis=-1)
    # f' is non-decreasing along the sorted knots up to rounding: the bracket is taken by position, not by value
    n_neg = np.sum(np.cumsum(g > 0.0, axis=-1) == 0, axis=-1)                 # knots before the first with f' > 0
    lo, hi = np.clip(n_neg - 1, 0, 7)[..., None], np.clip(n_neg, 0, 7)[..., None]
    t_lo, t_hi = np.take_along_axis(knots, lo, -1)[..., 0], np.take_along_axis(knots, hi, -1)[..., 0]
    g_lo, g_hi = np.take_along_axis(g, lo, -1)[..., 0], np.take_along_axis(g, hi, -1)[..., 0]
    den = g_hi - g_lo
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(den > 0.0, t_lo - g_lo * (t_hi - t_lo) / np.where(den > 0.0, den, 1.0), t_lo)
    t = np.where(n_neg == 0, 0.0, np.where(n_neg == 8, 1.0, np.clip(t, t_lo, t_hi)))
    x = a + t[..., None] * u
    return np.sqrt(np.sum(np.maximum(np.abs(x) - half, 0.0) ** 2, axis=-1))
