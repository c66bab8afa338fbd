"""envelope_line of vkvolume_amd/csrc/edt_passes.hpp restated in Python, statement by statement, with its two carries: DistanceCarry
(k_env_axis, edt_envelope.hip) and FeatureCarry (k_near_axis, nearest.hip).  Every intermediate is held to the range the kernel's types give
it and the stack-in-line inequalities are assertions.  tests/test_distance_weighted_cpu.py and tests/test_nearest_cpu.py hold it to the
min-plus line; no device is touched."""
NONE = 0xffffffff
UNWRITTEN = 0xA5A5A5A5


class DistanceCarry:
    """a position carries its capped distance (<= limit)"""

    def __init__(self, limit):
        self.limit = limit

    def skips(self, e):
        return e >= self.limit

    def g(self, e):
        return e

    def none(self):
        return self.limit

    def value(self, s, e, f):
        return min(self.limit, f)

    def store(self, dst, i, out):
        dst[i] = out


class FeatureCarry:
    """a position carries a feature or NONE; g_of(feature) is the lane's near_g, encode(s, feature) what the backward sweep writes; dist: None,
    or the line of d_dist2"""

    def __init__(self, limit, g_of, encode, dist=None):
        self.limit, self.g, self.encode, self.dist = limit, g_of, encode, dist

    def skips(self, e):
        return e == NONE

    def none(self):
        return NONE, self.limit

    def value(self, s, e, f):
        if f >= self.limit:
            return self.none()
        out = self.encode(s, e)
        assert out < NONE
        return out, f

    def store(self, dst, i, out):
        dst[i] = out[0]
        if self.dist is not None:
            self.dist[i] = out[1]


def envelope_line_py(src, w, carry):
    """one line of an axis pass: `src` the line of the source buffer, the returned list the line of the destination buffer, which holds the
    stack (entry k = s | t << 15 at position k) until the backward sweep overwrites it"""
    n = len(src)
    dst = [UNWRITTEN] * n

    def f(p, i, gi):
        wd = w * abs(p - i)
        assert wd <= 65535 and gi < 2 ** 32
        return gi + wd * wd        # < 2^33: 64 bits in the kernel

    k = s = t = gs = es = 0
    for u in range(n):
        eu = src[u]
        if carry.skips(eu):
            continue
        g = carry.g(eu)
        assert g < carry.limit        # a capped distance is skipped; the pass before stored no feature otherwise
        while k > 0 and f(t, s, gs) > f(t, u, g):
            k -= 1
            if k > 0:
                e = dst[k - 1]
                s, t = e & 0x7fff, e >> 15
                es = src[s]
                gs = carry.g(es)
        if k == 0:
            t = 0
        else:
            num, den = g + w * w * (u * u - s * s) - gs, 2 * w * w * (u - s)
            assert 0 <= num < 2 ** 34 and 0 < den < 2 ** 33 and u * u < 2 ** 32 and num // den >= t, (num, den, t)
            q = num // den
            if q >= n - 1:
                continue
            t = q + 1
        s, gs, es = u, g, eu
        assert k <= u and t >= k and t < 2 ** 16 and s <= 32767 and t <= 32767, (k, u, t)        # entry k lies at or below u and starts at or above k
        dst[k] = s | t << 15
        k += 1
    for u in range(n - 1, -1, -1):
        out = carry.none()
        if k > 0:
            assert t <= u and k - 1 <= t, (k, t, u)        # the top covers u, and the store at u hits no entry below the top
            out = carry.value(s, es, f(u, s, gs))
            if u == t:
                k -= 1
                if k > 0:
                    assert k - 1 < u
                    e = dst[k - 1]
                    s, t = e & 0x7fff, e >> 15
                    es = src[s]
                    gs = carry.g(es)
        carry.store(dst, u, out)
    assert k == 0
    return dst


def feature_line_py(src, w, limit, g_of, encode):
    """(the line of the destination feature buffer, the line of d_dist2) of a pass over features"""
    dist = [UNWRITTEN] * len(src)
    return envelope_line_py(src, w, FeatureCarry(limit, g_of, encode, dist)), dist
