"""The packed-state codec (TH_STATE_F16: tendrils_amd/csrc/th_packed.inc) value by value: an exact reference of encode and decode,
the value sets that walk every rounding boundary of it, and the layout of a value set as a state texture.  No GPU here.

The reference is written from the definition, independently of the numpy mirror in helpers.py (which it is there to check): it
takes an fp32 value apart into sign, exponent and mantissa - value = M * 2^E exactly, in int64 - and rounds the integer.
  position  q = clamp(rint_ties_even(x * 16384), -32767, 32767); x * 16384 is a power-of-two scaling, so rounding the exact
            product is what the device's fp32 multiply, clamp and rint compute (an overflowing product clamps either way);
            (x, y) = (-1e6, -1e6) is inert: the word (-32768, -32768); else a NaN in either component: (-32768, 0)
  velocity  IEEE binary16, round to nearest even: the quantum is 2^(p - 10) for a value with its leading bit at 2^p, p >= -14,
            and 2^-24 below (subnormals); a mantissa that rounds up to 2048 quanta carries into the exponent, and past the
            exponent 15 that is infinity - from 65520, the midpoint of 65504 and 2^16, on; NaN -> a quiet NaN of the same sign
Nothing on the encode side converts through np.float16.  Decode is exact by construction: short / 16384 and
(-1)^s (1024 + m) 2^(e - 25) (m 2^-24 for e = 0) in float64, both exactly representable in fp32."""
import numpy as np

F = np.float32
INERT = F(-1e6)
NAN_CODE = 0x7fc00000           # what probe() makes of any NaN
WIDTH = 250                     # of a laid-out value set: no multiple of 64


# ---- the exact reference ---------------------------------------------------------------------------------------------------------
def _parts(v):
    """fp32 array -> (negative, M, E, nan, inf) with |v| = M * 2^E exactly (int64) for the finite ones"""
    b = np.ascontiguousarray(v, F).view(np.uint32).astype(np.int64)
    e, m = (b >> 23) & 0xff, b & 0x7fffff
    M = np.where(e > 0, m | 0x800000, m)
    E = np.where(e > 0, e - 150, -149)
    return (b >> 31) != 0, M, E, (e == 255) & (m != 0), (e == 255) & (m == 0)


def _round_shift(M, shift):
    """rint_ties_even(M / 2^shift) for M < 2^24, shift >= 1 (beyond 26 the quotient is below a half whatever M is)"""
    shift = np.minimum(shift, 26)
    floor, rem, half = M >> shift, M & ((np.int64(1) << shift) - 1), np.int64(1) << (shift - 1)
    return floor + ((rem > half) | ((rem == half) & ((floor & 1) != 0)))


def encode_position(x):
    """fp32 -> the quantum count of ONE component, no sentinels: clamp(rint_ties_even(x * 16384), -32767, 32767); NaN -> 0"""
    neg, M, E, nan, inf = _parts(x)
    up = E + 14                                              # |x| * 16384 = M * 2^up
    whole = M << np.clip(up, 0, 16)                          # (M > 0 and up > 16: far beyond the clamp either way)
    q = np.where(up >= 0, whole, _round_shift(M, np.maximum(-up, 1)))
    q = np.where(inf | ((up > 16) & (M > 0)), 32767, np.minimum(q, 32767))
    return np.where(nan, 0, np.where(neg, -q, q)).astype(np.int64)


def encode_half(v):
    """fp32 -> the 16 bits of its binary16, round to nearest even (uint16)"""
    neg, M, E, nan, inf = _parts(v)
    lead = np.zeros(M.shape, np.int64)                       # the position of M's leading bit (M < 2^24)
    for k in range(1, 24):
        lead = np.where(M >> k != 0, k, lead)
    p = lead + E                                             # 2^p <= |v| < 2^(p + 1)
    normal = (p >= -14) & (M > 0)
    quantum = np.where(normal, p - 10, -24)
    shift = quantum - E                                      # >= 13 for an fp32 normal: 13 mantissa bits go
    n = _round_shift(M, np.maximum(shift, 1))                # in quanta: 1024 .. 2048 for a normal result, 0 .. 1024 below
    bits = np.where(normal, ((p + 15) << 10) + (n - 1024), n)
    bits = np.where(inf | (bits > 0x7c00), 0x7c00, bits)     # (n = 2048 carried into the exponent; exponent 31 is infinity)
    bits = np.where(nan, 0x7e00, bits)
    return (bits | np.where(neg, 0x8000, 0)).astype(np.uint16)


def decode_half(h):
    """the 16 bits of a binary16 -> fp32, exactly"""
    h = np.asarray(h).astype(np.int64)
    s, e, m = (h >> 15) & 1, (h >> 10) & 31, h & 0x3ff
    mag = np.where(e == 0, np.ldexp(m.astype(np.float64), -24), np.ldexp((1024 + m).astype(np.float64), e - 25))
    mag = np.where(e == 31, np.where(m == 0, np.inf, np.nan), mag)
    return np.where(s != 0, -mag, mag).astype(F)


def encode(st):
    """[..., 4] fp32 texels -> [..., 2] uint32 words"""
    st = np.asarray(st, F)
    x, y = st[..., 0], st[..., 1]
    inert = (x == INERT) & (y == INERT)
    nan = (np.isnan(x) | np.isnan(y)) & ~inert
    xs = np.where(inert | nan, -32768, encode_position(x))
    ys = np.where(inert, -32768, np.where(nan, 0, encode_position(y)))
    w0 = (xs & 0xffff) | ((ys & 0xffff) << 16)
    w1 = encode_half(st[..., 2]).astype(np.int64) | (encode_half(st[..., 3]).astype(np.int64) << 16)
    return np.stack([w0, w1], -1).astype(np.uint32)


def decode(words):
    """[..., 2] uint32 words -> [..., 4] fp32 texels: any word, also those encode() never writes"""
    w = np.asarray(words, np.uint32).astype(np.int64)
    xs, ys = w[..., 0] & 0xffff, w[..., 0] >> 16
    xs, ys = xs - ((xs & 0x8000) << 1), ys - ((ys & 0x8000) << 1)
    out = np.empty(w.shape[:-1] + (4,), F)
    out[..., 0] = (xs / 16384.0).astype(F)
    out[..., 1] = (ys / 16384.0).astype(F)                   # (ys = -32768 beside an ordinary xs: -2.0)
    inert = (xs == -32768) & (ys == -32768)
    nan = (xs == -32768) & ~inert
    out[inert, 0] = out[inert, 1] = INERT
    out[nan, 0] = out[nan, 1] = np.nan
    out[..., 2] = decode_half(w[..., 1] & 0xffff)
    out[..., 3] = decode_half(w[..., 1] >> 16)
    return out


def quantised(st):
    """what a packed ring holds of a state: decode(encode(.))"""
    return decode(encode(st))


def half_is_nan(h):
    h = np.asarray(h).astype(np.int64)
    return ((h & 0x7c00) == 0x7c00) & ((h & 0x3ff) != 0)


def words_equal(a, b):
    """[..., 2] words, bit for bit - a NaN half equal to any NaN half (bits_equal's rule: payloads are not pinned)"""
    a, b = np.asarray(a, np.uint32).astype(np.int64), np.asarray(b, np.uint32).astype(np.int64)
    lo = ((a[..., 1] & 0xffff) == (b[..., 1] & 0xffff)) | (half_is_nan(a[..., 1] & 0xffff) & half_is_nan(b[..., 1] & 0xffff))
    hi = ((a[..., 1] >> 16) == (b[..., 1] >> 16)) | (half_is_nan(a[..., 1] >> 16) & half_is_nan(b[..., 1] >> 16))
    return (a[..., 0] == b[..., 0]) & lo & hi


# ---- value sets --------------------------------------------------------------------------------------------------------------------
def _neighbours(v):
    v = np.atleast_1d(np.asarray(v, F))
    return np.concatenate([v, np.nextafter(v, F(np.inf)), np.nextafter(v, F(-np.inf))])


def _distinct(v):
    """one of each bit pattern, in the order of the bits"""
    return np.unique(np.ascontiguousarray(v, F).view(np.uint32)).view(F)


def velocity_values(distinct=True):
    """every finite fp16 value; every midpoint of two adjacent ones with its two fp32 neighbours; the overflow threshold, the
    subnormal range's ties, the extremes - all in both signs"""
    h = np.arange(0x10000, dtype=np.int64)
    finite = np.sort(decode_half(h[(h & 0x7c00) != 0x7c00]))
    mid64 = (finite[:-1].astype(np.float64) + finite[1:].astype(np.float64)) / 2
    mid = mid64.astype(F)
    assert (mid.astype(np.float64) == mid64).all()           # every midpoint is an fp32 value
    edges = np.array([65504.0, 1e30, np.inf, np.nan, 2.0 ** -25, np.nextafter(F(2.0 ** -25), F(1)), 2.0 ** -24, 2.0 ** -149,
                      0.0], F)
    v = np.concatenate([finite, _neighbours(mid), _neighbours(F(65520.0)), edges])
    v = np.concatenate([v, -v])
    return _distinct(v) if distinct else v


NEAR_ZERO = np.array([0.0, -0.0, 1e-6, -1e-6, -1e-30], F)


def position_values(distinct=True):
    """the 65 538 ties (k + 0.5) / 16384, k = -32769 .. 32768, with their two fp32 neighbours; zeros and what rounds to them;
    what the clamp catches; -1e6 (inert only as a pair) and its neighbours"""
    k = np.arange(-32769, 32769, dtype=np.float64)
    tie64 = (k + 0.5) / 16384
    tie = tie64.astype(F)
    assert (tie.astype(np.float64) == tie64).all()           # every tie is an fp32 value
    v = np.concatenate([_neighbours(tie), NEAR_ZERO, np.array([2.5, -2.5, np.inf, -np.inf, 1e30, -1e30], F), _neighbours(INERT)])
    return _distinct(v) if distinct else v


# position pairs that meet the sentinels: inert needs both components, a NaN in either makes both NaN, -1e6 beside anything
# else is an ordinary (clamped) value
PAIRINGS = np.array([[-1e6, -1e6], [-1e6, 0.3], [0.3, -1e6], [np.nan, 0.3], [0.3, np.nan], [-1e6, np.nan], [np.nan, -1e6],
                     [np.nan, np.nan], [np.nextafter(INERT, F(0)), -1e6], [-1e6, np.nextafter(INERT, F(-np.inf))]], F)


def negative_zero_positions(v):
    """the values whose scaled, clamped, rounded position is -0.0: the negatives of magnitude up to half a quantum, -0.0 itself"""
    v = np.asarray(v, F)
    return np.signbit(v) & (v >= F(-2.0 ** -15))


def raw_words():
    """[n, 2] words to decode: every 16-bit pattern in each of the four half-word places (four different walks of the 65 536,
    side by side), then the NaN-position sentinel beside every ys - which holds (-32768, -32768), inert - ; the first walk
    holds (xs != -32768, ys = -32768) words, which pack_state never writes"""
    i = np.arange(0x10000, dtype=np.int64)
    ys = (i * 40503 + 17) & 0xffff                           # (an odd multiplier: a walk of all 65 536)
    hx = (i * 25173 + 13849) & 0xffff
    hy = 0xffff - i
    walk = np.stack([i | (ys << 16), hx | (hy << 16)], -1)
    for part in (i, ys, hx, hy):
        assert len(np.unique(part)) == 0x10000
    assert ((ys == 0x8000) & (i != 0x8000)).any()
    sentinel = np.stack([0x8000 | (i << 16), hy | (hx << 16)], -1)
    return np.concatenate([walk, sentinel]).astype(np.uint32)


# ---- layout --------------------------------------------------------------------------------------------------------------------------
def shape_for(count, width=WIDTH):
    """(w, h) of the smallest texture of this width that holds `count` texels and is no multiple of 256 texels"""
    h = -(-count // width)
    while (h * width) % 256 == 0:
        h += 1
    assert width % 64 != 0
    return width, h


def lay_out(texels, shape=None, pad=(INERT, INERT, 0.0, 0.0)):
    """[n, 4] texels -> [h, w, 4] state, the rest inert"""
    texels = np.asarray(texels, F)
    w, h = shape or shape_for(len(texels))
    assert len(texels) <= w * h
    out = np.empty((h * w, 4), F)
    out[:] = np.array(pad, F)
    out[:len(texels)] = texels
    return out.reshape(h, w, 4)


def lay_out_words(words):
    """[n, 2] words -> [h, w, 2], the rest the inert word with zero velocity"""
    words = np.asarray(words, np.uint32)
    w, h = shape_for(len(words))
    out = np.empty((h * w, 2), np.uint32)
    out[:] = (0x80008000, 0)
    out[:len(words)] = words
    return out.reshape(h, w, 2)


def _cycled(v, n, backwards=False):
    k = np.arange(n) % len(v)
    return v[len(v) - 1 - k] if backwards else v[k]


def special_texels():
    """the sentinel pairings and every pair of near-zero positions, over velocities around zero"""
    near = np.concatenate([NEAR_ZERO, np.array([1e-30], F), _neighbours(F(-2.0 ** -15)), _neighbours(F(2.0 ** -15))])
    around = np.array([0.0, -0.0, 2.0 ** -25, -2.0 ** -25, 2.0 ** -24, 2.0 ** -149, -1e-8, 65520.0, np.nan, -np.inf], F)
    gx, gy = np.meshgrid(near, near)
    pos = np.concatenate([PAIRINGS, np.stack([gx.ravel(), gy.ravel()], -1)])
    vel = np.stack([_cycled(around, len(pos)), _cycled(around, len(pos), backwards=True)], -1)
    return np.concatenate([pos, vel], -1).astype(F)


def full_texels():
    """[n, 4]: every position value in x and (in the opposite order) in y, every velocity value in z and (opposite) in w, behind
    the special texels - the smallest state through which every value of both sets passes in both halves of both words"""
    pos, vel = position_values(), velocity_values()
    n = max(len(pos), len(vel))
    body = np.stack([_cycled(pos, n), _cycled(pos, n, True), _cycled(vel, n), _cycled(vel, n, True)], -1)
    return np.concatenate([special_texels(), body]).astype(F)


def sample_texels(count):
    """[count, 4]: the special texels, then an even sample of full_texels()' body - for the small shapes"""
    special, body = special_texels(), full_texels()[len(special_texels()):]
    assert count > len(special)
    pick = np.linspace(0, len(body) - 1, count - len(special)).astype(np.int64)
    return np.concatenate([special, body[pick]]).astype(F)


# ---- the probe: all 32 bits of one component as numbers the codec leaves alone -------------------------------------------------------
def probe(st, component):
    """bits 0-14 of st[..., component] as the x quantum, bits 15-29 as the y quantum, bits 30-31 as the velocity z (0 .. 3), the
    component as w; NAN_CODE for any NaN.  Every result is a fixed point of the codec."""
    v = np.ascontiguousarray(np.asarray(st, F)[..., component])
    b = np.where(np.isnan(v), NAN_CODE, v.view(np.uint32).astype(np.int64))
    out = np.empty(v.shape + (4,), F)
    out[..., 0] = (b & 0x7fff) / 16384.0
    out[..., 1] = ((b >> 15) & 0x7fff) / 16384.0
    out[..., 2] = b >> 30
    out[..., 3] = component
    return out


# the same in HIP: a device function both program forms call
PROBE_TEXT = """struct Probe { int plant_step; int component; };
__device__ float4 probe(float4 self, int component)
{
    const float v = component == 0 ? self.x : component == 1 ? self.y : component == 2 ? self.z : self.w;
    const unsigned b = v != v ? 0x7fc00000u : __float_as_uint(v);
    return make_float4((float)(b & 0x7fffu) * 6.103515625e-05f, (float)((b >> 15) & 0x7fffu) * 6.103515625e-05f,
                       (float)(b >> 30), (float)component);
}
"""
# as a state program: one pass probes the newest state
STATE_PROBE = PROBE_TEXT + """__device__ float4 th_main(const th_pass &p)
{
    return probe(p.self, th_uniforms<Probe>(p).component);
}
"""
# as a step program: plants its targets texel at step plant_step, probes at the step after, carries the state elsewhere
# (plant_step = -1: the first step probes what the ring holds)
STEP_PLANT_PROBE = PROBE_TEXT + """__device__ float4 th_step_main(const th_step_pass &s)
{
    const Probe &u = th_uniforms<Probe>(s);
    if ((int)s.step == u.plant_step) return th_targets(s);
    if ((int)s.step == u.plant_step + 1) return probe(s.self, u.component);
    return s.self;
}
"""


def plant_probe_states(start, targets, n, plant_step, component):
    """states 0 .. n of STEP_PLANT_PROBE on a packed ring, in numpy: the exact reference's quantised() after every step (a step
    that carries the state quantises a quantised state: checked to change no bit once per distinct state, not recomputed)"""
    states, carried = [quantised(start)], set()
    for k in range(n):
        cur = states[-1]
        if k == plant_step:
            states.append(quantised(targets))
        elif k == plant_step + 1:
            states.append(quantised(probe(cur, component)))
        else:
            if id(cur) not in carried:
                again = quantised(cur)
                assert ((again.view(np.uint32) == cur.view(np.uint32)) | (np.isnan(again) & np.isnan(cur))).all()
                carried.add(id(cur))
            states.append(cur)
    return states
