"""The packed-state codec on the GPU (TH_STATE_F16; tendrils_amd/csrc/th_packed.inc: unpack_state, pack_state, quantize_state),
value by value against the exact reference of packed_codec_cases.py - every finite fp16 value, every fp16 midpoint and every
position tie with their fp32 neighbours, the overflow and underflow thresholds, the clamp, the sentinels, every 16-bit pattern
of each half-word:
  decode   raw words written straight into a packed ring buffer; what Particles.read() gives, what a step program sees as
           s.self and what a state program sees as p.self (a PROBE program that tells all 32 bits of one component as numbers
           the codec leaves alone)
  encode   upload_texels of the value sets; the raw words read back
  carry    the state a fused launch carries between two steps in registers (quantize_state) is the stored texel, decoded: a
           PLANT / PROBE step program plants unquantised fp32 values inside a launch and tells the bits the next step sees;
           fused against unfused (fuse = 0), n calls of one step and numpy, on both ring buffers; once more on a ring the
           built-in integrator left tile-sorted
Every comparison is on the bits (bits_equal: NaN equals NaN whatever its payload; a NaN half equals a NaN half) and over every
texel.

Shapes: 50 x 30 (1500 texels: no multiple of 64 or 256) with the sentinel pairings and the near-zero values, and the smallest
250-wide textures that hold the value sets (250 x 1017, 250 x 525: more than one workgroup, no multiple of 256 texels).  The
programs are compiled and the sets built once for the module; nothing here writes a set."""
import ctypes as C

import numpy as np
import pytest

from tendrils_amd import _capi, sharding
from tendrils_amd._capi import call
from tendrils_amd.particles import Program, StepProgram, run_pass, run_step_program

import packed_codec_cases as cases
from helpers import bits_equal
from test_gpu_step_program import DT, H, TIMES, W, context, device_ptrs, state
import test_gpu_step_program_slots as slots

pytestmark = pytest.mark.gpu

F = np.float32
# (n, plant_step): the carry inside a launch; then a carried echo; inside the first of two launches; across the split at 32
CARRIES = ((2, 0), (3, 0), (33, 30), (33, 31))


class ProbeU(C.Structure):
    _fields_ = [("plant_step", C.c_int32), ("component", C.c_int32)]


@pytest.fixture(scope="module")
def programs():
    progs = dict(step=StepProgram.from_source(cases.STEP_PLANT_PROBE, ProbeU, name="plant_probe"),
                 state=Program.from_source(cases.STATE_PROBE, ProbeU, name="probe"))
    yield progs
    for p in progs.values():
        p.dispose()


@pytest.fixture(scope="module")
def sets():
    full = cases.lay_out(cases.full_texels())
    out = dict(full=full, small=cases.lay_out(cases.sample_texels(W * H - 7), (W, H)), words=cases.lay_out_words(cases.raw_words()),
               sorted=cases.lay_out(cases.sample_texels(slots.N * slots.N - 7), (slots.N, slots.N)))
    out["start_small"] = state(W, H, seed=5)
    out["start_full"] = np.ascontiguousarray(full[::-1, ::-1])           # (another texel's values: a plant that did nothing shows)
    for v in out.values():
        v.setflags(write=False)
    return out


def shape_of(st):
    return st.shape[1], st.shape[0]


def raw_view(p, buffer):
    """ring buffer `buffer` of a packed ring as the device holds it: [texels, 2] words (int32: the bits)"""
    d = C.c_void_p()
    call("th_state_device_ptr", p._ctx, int(buffer), C.byref(d))
    return sharding.device_view(d.value, (p.shape[0] * p.shape[1], 2), "<i4")


def write_words(p, words):
    """the words into every ring buffer, behind the codec's back"""
    import torch
    flat = torch.from_numpy(words.reshape(-1, 2).view(np.int32).copy())      # (a copy: the sets are read-only)
    for k in range(len(p.buffers)):
        raw_view(p, k).copy_(flat)
    torch.cuda.synchronize()
    p.sync()


def read_words(p, buffer):
    p.sync()
    return raw_view(p, buffer).cpu().numpy().view(np.uint32).reshape(p.shape[1], p.shape[0], 2)


def upload_targets(p, tg):
    call("th_targets_upload", p._ctx, np.ascontiguousarray(tg, F).ctypes.data_as(_capi._fp))


def run(p, programs, n, plant_step, component, first=0):
    run_step_program(p, programs["step"], dict(plant_step=plant_step, component=component), TIMES[first:first + n], DT, n)


def differing(got, want):
    bad = ~bits_equal(got, want).all(-1)
    return int(bad.sum()), got[bad][:4], want[bad][:4]


# ---- 1. decode ---------------------------------------------------------------------------------------------------------------------------
def test_every_word_decodes_as_the_exact_reference(sets):
    words = sets["words"]
    want = cases.decode(words)
    p = context(*shape_of(words), packed=True)
    write_words(p, words)
    for k in range(2):
        assert (read_words(p, k) == words).all()                          # (the words did land as they are)
        got = p.read(k)
        assert bits_equal(got, want).all(), differing(got, want)
    p.dispose()


# ---- 2. encode ---------------------------------------------------------------------------------------------------------------------------
def test_every_value_encodes_as_the_exact_reference(sets):
    for name in ("full", "small"):
        st = sets[name]
        want = cases.encode(st)
        p = context(*shape_of(st), packed=True)
        p.upload_texels(st, -1)
        for k in range(2):
            got = read_words(p, k)
            same = cases.words_equal(got, want)
            assert same.all(), (name, k, int((~same).sum()), st[~same][:4], got[~same][:4], want[~same][:4])
        got, back = p.read(0), cases.decode(want)
        assert bits_equal(got, back).all(), differing(got, back)           # and read() undoes it as the reference does
        p.dispose()


# ---- 3. a program's view of the ring is the decode ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("component", range(4))
def test_a_program_sees_the_decode_of_the_stored_words(programs, sets, component):
    words = sets["words"]
    decoded = cases.decode(words)
    want = cases.probe(decoded, component)
    assert bits_equal(cases.quantised(want), want).all()                  # (the probe's numbers pass the codec unchanged)
    # one PROBE step of the step program - fused, in place - and of the staged single-step path
    for fuse in (None, 0):
        p = context(*shape_of(words), packed=True, fuse=fuse)
        write_words(p, words)
        run(p, programs, 1, -1, component)
        got = p.read(0)
        assert bits_equal(got, want).all(), (fuse,) + differing(got, want)
        assert bits_equal(p.read(1), decoded).all()                       # (state 0 stays what it was)
        p.dispose()
    # the same probe as a state program
    p = context(*shape_of(words), packed=True)
    write_words(p, words)
    run_pass(p, programs["state"], dict(component=component), _capi.TH_TARGET_RING)
    got = p.read(0)
    assert bits_equal(got, want).all(), differing(got, want)
    p.dispose()


# ---- 4. the fused carry is the stored texel ---------------------------------------------------------------------------------------------------
def carried(programs, start, targets, n, plant_step, component):
    """(state n, state n - 1) of the PLANT / PROBE call three ways: fused, fuse = 0, n calls of one step"""
    out = []
    for way in ("fused", "staged", "single"):
        p = context(*shape_of(start), packed=True, fuse=0 if way == "staged" else None)
        p.upload_texels(start, -1)
        upload_targets(p, targets)
        before = device_ptrs(p)
        if way == "single":
            for k in range(n):
                run(p, programs, 1, plant_step - k, component, first=k)   # (a call's step index starts at 0)
        else:
            run(p, programs, n, plant_step, component)
        assert device_ptrs(p) == (before if n % 2 == 0 else before[::-1])
        out.append((p.read(0), p.read(1)))
        p.dispose()
    return out


def held_to_the_stored_texel(programs, start, targets, n, plant_step, component):
    planted = targets[..., component]
    if component < 2:
        # the class the closed form once got wrong - a fix is only tested if the case is present
        assert ((planted > F(-2.0 ** -15)) & (planted < 0)).sum() >= 3 and cases.negative_zero_positions(planted).sum() >= 5
    with np.errstate(all="ignore"):
        want = cases.plant_probe_states(start, targets, n, plant_step, component)
    fused, staged, single = carried(programs, start, targets, n, plant_step, component)
    for k in range(2):
        ref = want[n - k]
        assert bits_equal(fused[k], staged[k]).all(), ("fused / fuse = 0", k) + differing(fused[k], staged[k])
        assert bits_equal(fused[k], single[k]).all(), ("fused / n calls", k) + differing(fused[k], single[k])
        assert bits_equal(fused[k], ref).all(), ("fused / numpy", k) + differing(fused[k], ref)
        assert bits_equal(staged[k], ref).all(), ("fuse = 0 / numpy", k) + differing(staged[k], ref)
    # the probe did tell: what it left is neither the start nor the planted state
    assert (~bits_equal(fused[0], cases.quantised(targets))).any() and (~bits_equal(fused[0], cases.quantised(start))).any()


@pytest.mark.parametrize("component", range(4))
@pytest.mark.parametrize("n,plant_step", CARRIES)
def test_the_fused_carry_is_the_stored_texel(programs, sets, n, plant_step, component):
    """On quantize_state as it stood - rint(..) * 2^-14 - this fails for components 0 and 1 wherever the carry stays in registers
    ((2, 0), (3, 0), (33, 30)): the planted positions in [-2^-15, -0.0] reach the probe as -0.0 (bit 31 set: z = 2) fused and as
    +0.0 (z = 0) on the three other paths.  (33, 31) carries the planted state through memory and passed before."""
    held_to_the_stored_texel(programs, sets["start_small"], sets["small"], n, plant_step, component)


@pytest.mark.parametrize("component", range(4))
@pytest.mark.parametrize("n,plant_step", ((3, 0), (33, 30)))
def test_every_rounding_boundary_passes_through_the_fused_carry(programs, sets, n, plant_step, component):
    """the same at the value-set shape: every value of both sets goes through quantize_state, not only through pack_state"""
    held_to_the_stored_texel(programs, sets["start_full"], sets["full"], n, plant_step, component)


# ---- 5. tile-sorted slots ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("component", range(4))
def test_the_carry_on_a_ring_the_built_in_integrator_left_tile_sorted(programs, sets, component):
    targets = sets["sorted"]
    assert cases.negative_zero_positions(targets[..., :2]).sum() >= 8
    got = {}
    for bucket in (1, 0):
        p = slots.context(bucket=bucket, packed=True)
        p.upload_texels(slots.fast_state(), -1)
        slots.builtin_steps(p)
        upload_targets(p, targets)
        order = slots.slot_order(p)[0]
        run(p, programs, 3, 0, component)
        got[bucket] = (order, p.read(0), p.read(1))
        p.dispose()
    assert got[1][0] > 0 and got[0][0] == 0                               # the built-in steps did sort the one
    # plant, probe, carry: states 3 and 2 are the probe of the planted state, whatever the built-in steps left
    with np.errstate(all="ignore"):
        want = cases.quantised(cases.probe(cases.quantised(targets), component))
    for bucket in (1, 0):
        for k in (1, 2):
            assert bits_equal(got[bucket][k], want).all(), (bucket, k) + differing(got[bucket][k], want)
