"""The test-only harness around the shared primitives (tests/native/: exclusive scan, texel-set rank, radix sort, block_scan - linked
against the object the product library ships) as numpy-in / numpy-out functions, and the plain numpy references the GPU
tests compare with: tests/test_gpu_prims.py, tests/test_gpu_statistics.py; the references themselves are pinned on
hand-made inputs by tests/test_prims_build.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
LIB_PATH = os.environ.get("TH_PRIMS_LIB") or os.path.join(NATIVE, "_build", "libth_prims.so")   # TH_PRIMS_LIB: diagnostic builds
SORT_OBJECT = os.path.join(ROOT, "tendrils_amd", "lib", "obj", "th_sort.o")
ENTRY_POINTS = ["thp_block_scan", "thp_exclusive_scan_u32", "thp_last_error", "thp_radix_sort_empty", "thp_radix_sort_u32",
                "thp_radix_sort_u64", "thp_texel_set_rank"]
RADIX_BITS = 8          # th_kernels.hpp: kRadixBits

_u32p, _u64p, _i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int)
_PROTOTYPES = {
    "thp_last_error": (C.c_char_p, []),
    "thp_exclusive_scan_u32": (C.c_int, [_u32p, C.c_uint32]),
    "thp_texel_set_rank": (C.c_int, [_u64p, C.c_uint32, _u32p, _u32p, _u64p]),
    "thp_radix_sort_u32": (C.c_int, [_u32p, _u32p, C.c_uint32, C.c_int, C.c_int, _u32p, _u32p, _i32p]),
    "thp_radix_sort_u64": (C.c_int, [_u64p, _u32p, C.c_uint32, C.c_int, C.c_int, _u64p, _u32p, _i32p]),
    "thp_radix_sort_empty": (C.c_int, [C.c_int, C.c_uint32, C.c_int, C.c_int, _i32p]),
    "thp_block_scan": (C.c_int, [C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
}
_lib = None


class PrimsError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("prims harness code %d: %s" % (code, message))
        self.code = code


def build():
    """make the harness (the product's objects first, when they are missing: it links lib/obj/th_sort.o)"""
    if not os.path.exists(SORT_OBJECT):
        import __graft_entry__ as g
        g.build()
    subprocess.check_call(["make", "-C", NATIVE, "all"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def load():
    """The product library first (tendrils_amd._capi.load: the process keeps ONE ROCm runtime), then the harness."""
    global _lib
    if _lib is None:
        from tendrils_amd import _capi
        _capi.load()
        if not os.path.exists(LIB_PATH):
            build()
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def _call(name, *args):
    lib = load()
    code = getattr(lib, name)(*args)
    if code != 0:
        raise PrimsError(code, lib.thp_last_error().decode(errors="replace"))


# ---- the primitives, host arrays in and out ---------------------------------------------------------------------------
def exclusive_scan_u32(data):
    out = np.array(data, np.uint32, copy=True, order="C")
    _call("thp_exclusive_scan_u32", out.ctypes.data_as(_u32p), out.size)
    return out


def texel_set_rank(mask, counts=None):
    """mask: uint64 words, bit t & 63 of word t >> 6 is texel t; counts: what a caller's kernel left as the words' counts - the
    launcher only scans them - or None: it counts the mask's bits.  -> (the members before each word, the members)"""
    mask = np.ascontiguousarray(mask, np.uint64)
    given = None if counts is None else np.ascontiguousarray(counts, np.uint32)
    assert given is None or given.shape == mask.shape
    out, total = np.empty(mask.size, np.uint32), C.c_uint64(0)
    _call("thp_texel_set_rank", mask.ctypes.data_as(_u64p), mask.size, None if given is None else given.ctypes.data_as(_u32p),
          out.ctypes.data_as(_u32p), C.byref(total))
    return out, total.value


def radix_sort(keys, vals, begin_bit, end_bit):
    """keys: uint32 or uint64 array; vals: uint32 array or None (iota).  -> (keys_out, vals_out, in_b)"""
    keys = np.ascontiguousarray(keys)
    assert keys.dtype in (np.uint32, np.uint64) and keys.ndim == 1
    kp = _u32p if keys.dtype == np.uint32 else _u64p
    keys_out, vals_out, in_b = np.empty_like(keys), np.empty(keys.size, np.uint32), C.c_int(-1)
    vp = None
    if vals is not None:
        vals = np.ascontiguousarray(vals, np.uint32)
        assert vals.shape == keys.shape
        vp = vals.ctypes.data_as(_u32p)
    _call("thp_radix_sort_u32" if keys.dtype == np.uint32 else "thp_radix_sort_u64", keys.ctypes.data_as(kp), vp, keys.size,
          begin_bit, end_bit, keys_out.ctypes.data_as(kp), vals_out.ctypes.data_as(_u32p), C.byref(in_b))
    return keys_out, vals_out, in_b.value


def radix_sort_empty(key_bytes, cap, begin_bit, end_bit):
    """n = 0 over buffers of cap elements: raises when a buffer was written; -> in_b"""
    in_b = C.c_int(-1)
    _call("thp_radix_sort_empty", key_bytes, cap, begin_bit, end_bit, C.byref(in_b))
    return in_b.value


def block_scan(N, values):
    """values: [rounds, N] uint32 or uint64 -> (exclusive prefixes [rounds, N], the total every thread was handed [rounds, N])"""
    values = np.ascontiguousarray(values)
    assert values.dtype in (np.uint32, np.uint64) and values.ndim == 2 and values.shape[1] == N
    out, totals = np.empty_like(values), np.empty_like(values)
    _call("thp_block_scan", N, values.dtype.itemsize, values.ctypes.data, out.ctypes.data, totals.ctypes.data, values.shape[0])
    return out, totals


# ---- references ---------------------------------------------------------------------------------------------------------
def scan_reference(data):
    """exclusive prefix sums mod 2^32 (the running sum in uint64: 2^32 words of < 2^32 cannot wrap it)"""
    running = np.cumsum(np.asarray(data, np.uint32).astype(np.uint64))
    out = np.zeros(running.size, np.uint64)
    out[1:] = running[:-1]
    return (out & np.uint64(0xffffffff)).astype(np.uint32)


def texel_set_reference(mask):
    """the members before each word - the exclusive scan of the words' popcounts - and the members"""
    bits = np.unpackbits(np.ascontiguousarray(mask, np.uint64).view(np.uint8)).reshape(-1, 64)
    return scan_reference(bits.sum(axis=1)), int(bits.sum())


def block_scan_reference(values):
    """per row: exclusive prefixes and the total, in the element type's own modular arithmetic"""
    values = np.asarray(values)
    with np.errstate(over="ignore"):
        incl = np.cumsum(values, axis=1, dtype=values.dtype)
    return incl - values, incl[:, -1]


def sort_digits(keys, begin_bit, end_bit):
    keys = np.asarray(keys)
    mask = keys.dtype.type((1 << (end_bit - begin_bit)) - 1)
    return (keys >> keys.dtype.type(begin_bit)) & mask


def sort_reference(keys, vals, begin_bit, end_bit):
    """stable sort by key bits [begin_bit, end_bit): whole keys and values in the new order; vals None = positions"""
    keys = np.asarray(keys)
    vals = np.arange(keys.size, dtype=np.uint32) if vals is None else np.asarray(vals, np.uint32)
    perm = np.argsort(sort_digits(keys, begin_bit, end_bit), kind="stable")
    return keys[perm], vals[perm]


def sort_passes(begin_bit, end_bit):
    """passes of the plan a bit range implies: digits of at most RADIX_BITS bits; the result lies in buffer passes & 1"""
    return -(-(end_bit - begin_bit) // RADIX_BITS)


INERT = np.float32(-1e6)
FLT_MAX = np.finfo(np.float32).max


def stats_reference(texels, limit):
    """th_counters of a state (include/tendrils_hip.h), from its description:
    live      x or y differs from -1e6 (a NaN differs)
    nan       any of the four components is NaN, inert or not
    speed     sqrt(z*z + w*w), every operation rounded to float32
    finite    live, not nan, speed <= FLT_MAX - the particles sum_speed and max_speed are taken over
    capped    finite and speed >= float32(limit) * float32(1 - 2^-20), the product in float32
    sum_speed math.fsum of the finite speeds (correctly rounded); max_speed their maximum, 0 without any."""
    t = np.ascontiguousarray(texels, np.float32).reshape(-1, 4)
    x, y, z, w = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    live = (x != INERT) | (y != INERT)
    nan = np.isnan(x) | np.isnan(y) | np.isnan(z) | np.isnan(w)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        speed = np.sqrt(z * z + w * w)
        assert speed.dtype == np.float32
        finite = live & ~nan & (speed <= FLT_MAX)
        cap = np.float32(limit) * np.float32(1.0 - 2.0 ** -20)
        capped = finite & (speed >= cap)
    fs = speed[finite]
    return dict(particles=t.shape[0], live=int(live.sum()), nan=int(nan.sum()), capped=int(capped.sum()),
                sum_speed=math.fsum(fs.astype(np.float64).tolist()), max_speed=float(fs.max()) if fs.size else 0.0)


def sum_speed_bound(want):
    """Non-negative doubles added in some order: |got - fsum| <= N * 2^-53 * fsum, N the particle count (derived, not measured)."""
    return want["particles"] * 2.0 ** -53 * want["sum_speed"]


def assert_counters(got, want, what):
    """every counter exactly, sum_speed within sum_speed_bound; the message names the wrong counter"""
    for k in ("particles", "live", "nan", "capped", "max_speed"):
        assert got[k] == want[k], "%s: %s = %r, reference %r" % (what, k, got[k], want[k])
    err, bound = abs(got["sum_speed"] - want["sum_speed"]), sum_speed_bound(want)
    assert err <= bound, "%s: sum_speed = %r, reference %r: off by %.3g, bound %.3g" % (what, got["sum_speed"], want["sum_speed"], err, bound)
