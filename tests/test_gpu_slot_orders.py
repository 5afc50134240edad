"""The transitions between slot orders that no other suite forces (th_order.hip: ring_trade and its callers; th_step.hip: the
slot plan of a single step, the route of a fused launch; the th_kernel_timing bracket).  Every test runs two contexts on the
same inputs - one over tile-sorted slots or fused launches, one without - and compares both ring buffers bit for bit (and the
flow texture where it draws): a slot order is invisible in every result.  The counters th_slot_order reports are asserted as
constants: the sorts these sequences start and the buffers they leave in a sorted order."""
import ctypes as C

import numpy as np
import pytest

from helpers import bits_equal
from test_gpu_async_sort import loop_inputs, sorts

pytestmark = pytest.mark.gpu

N, VIEW = 128, (96, 54)          # (the shape of test_gpu_async_sort.py: sorting is possible there under bucket = 1)


def make(st, packed=False, pipeline=None, **options):
    import tendrils_amd as ta
    from tendrils_amd.tendrils import View
    opts = ta.defaults()
    if packed:
        opts["stateFormat"] = ta.TH_STATE_F16
    t = ta.Tendrils(View(*VIEW), opts)
    t.resize()
    t.setup(N)
    for name, value in options.items():
        t.particles.option(name, value)
    if pipeline:
        t.particles.draw_pipeline(pipeline)
    t.particles.upload_texels(st)
    t.timer.time = 3000.0
    return t


def same_ring(a, b):
    return bits_equal(a.particles.read(0), b.particles.read(0)).all() and bits_equal(a.particles.read(1), b.particles.read(1)).all()


def test_packed_ring_steps_over_sorted_slots():
    """TH_STATE_F16 under bucket 1: every second step() re-sorts by a plain move of its input into the spare buffer, which takes
    the input's place in the ring (enqueue_step: the packed re-sort)."""
    st = loop_inputs(N, VIEW, 31)
    a = make(st, packed=True, bucket=1, resort_steps=2)
    b = make(st, packed=True, bucket=0, resort_steps=2)
    for _ in range(7):
        for t in (a, b):
            t.timer.tick()
            t.step()
    got = sorts(a), sorts(b)                               # (a read-back by texel restores texel order: ask first)
    print("packed ring, 7 steps: (sorts, sorted_buffers) sorted | texel order", got)
    assert got == ((4, 2), (0, 0))
    assert same_ring(a, b)
    assert a.particles.read(0).any()
    a.dispose(); b.dispose()


def test_two_orders_meet_a_draw():
    """five steps without a draw re-sort inside the steps, output alone: the ring's two buffers end up in different orders, and
    the draw over the slots brings ring[1] into ring[0]'s (align_slot_orders: out of its own order, into the other)"""
    st = loop_inputs(N, VIEW, 32)
    a = make(st, pipeline="bins", bucket=1, resort_steps=2, async_sort=0)
    b = make(st, pipeline="bins", bucket=0, resort_steps=2, async_sort=0)
    for _ in range(5):
        for t in (a, b):
            t.timer.tick()
            t.step()
    before = sorts(a)
    for t in (a, b):
        t.draw()
    met = sorts(a)
    assert a.fragments == b.fragments > 0
    for _ in range(2):
        for t in (a, b):
            t.timer.tick()
            t.step().draw()
        assert a.fragments == b.fragments > 0
    got = before, met, sorts(a), sorts(b)
    print("two orders meet a draw: (sorts, sorted_buffers) after 5 steps | after the draw | after 2 more frames | texel order", got)
    assert got == ((3, 2), (3, 2), (4, 2), (0, 0))
    assert same_ring(a, b)
    assert bits_equal(a.flow.read(), b.flow.read()).all() and a.flow.read().any()
    a.dispose(); b.dispose()


def test_fused_chunks_of_odd_and_single_length():
    """step_n(33) is a launch of 32 steps and one of a single step, whose state m - 1 is its own input; step_n(65) two of 32 and
    one more single: the ring flips behind every odd launch, and the slots are re-sorted in front of every call"""
    st = loop_inputs(N, VIEW, 33)
    a = make(st, fuse=1, bucket=1, rebucket_steps=2)
    b = make(st, fuse=0, bucket=1, rebucket_steps=2)
    for n in (33, 65):
        for t in (a, b):
            t.step_n(n)
        assert same_ring(a, b)
    assert a.timer.time == b.timer.time and a.particles.read(0).any()
    a.dispose(); b.dispose()


def timed(t):
    from tendrils_amd import _capi
    ms, launches = C.c_float(-1.0), C.c_int32(-1)
    _capi.call("th_kernel_timing_read", t.particles._ctx, C.byref(ms), C.byref(launches))
    return ms.value, launches.value


def test_kernel_timing_brackets_every_launch_outside_a_capture():
    from tendrils_amd import _capi
    st = loop_inputs(N, VIEW, 34)
    a = make(st)                                            # (the plain two-buffer f32 ring; 128^2 particles never sort by themselves)
    b = make(st, fuse=0, graph=1)
    for t in (a, b):
        _capi.call("th_kernel_timing", t.particles._ctx, 1)
        for _ in range(3):
            t.timer.tick()
            t.step()
    for t in (a, b):
        t.step_n(40)                                        # fused: 32 + 8 steps, two launches; captured: none bracketed
    ms, launches = timed(a)
    print("kernel timing: fused context %d launches, mean %.5f ms" % (launches, ms))
    assert launches == 3 + 2 and ms > 0.0
    ms, launches = timed(b)
    print("kernel timing: captured context %d launches, mean %.5f ms" % (launches, ms))
    assert launches == 3 and ms > 0.0
    assert same_ring(a, b)
    a.dispose(); b.dispose()
