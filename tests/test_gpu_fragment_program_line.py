"""The fragment's line on the GPU (th_line(f): include/tendrils_hip.h "fragment programs"; tendrils_amd/csrc/th_fragline.hip, the
line entry points of th_fragment_prelude.inc).  No expected value comes from the code under test.  `along` is checked against the
library's own interpolation: with a vertex colour of 0 at a line's first vertex and 1 at its second the varying IS the parameter,
so color.x - along is exactly 0 wherever a line drew.  `line`, `across` and `length` are restated here per fragment from the key
the EXISTING emits hand out (stream index in the low word, texel above it) and the line's endpoints - the state itself under a
vertex program that passes xy through, the vertex positions of the trail export under the built-in stage - snapped in numpy's
fp32 and carried on in Python integers; the restated fragments are blended by the existing merges.  Every comparison is bit for
bit on the flow field and on the emitted varyings, byte for byte on the RGBA8 view."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import GOLDEN, bits_equal, deposit_hashed_inputs, load
from test_fragment_program_build import VIGNETTE, FragUniforms
from test_gpu_draw_program import FlowUniforms
from test_gpu_fragment_program import (base_flow, color_map, kernel_launches, last_draw, make, same, sorted_buffers, stages_run,
                                       tap_nearest, target, uniforms_of)

pytestmark = pytest.mark.gpu

FLOW_PASS, VIEW_PASS = 0, 1          # TH_PASS_FLOW, TH_PASS_VIEW
STREAM, BINS = 0, 1                  # TH_DRAW_STREAM, TH_DRAW_BINS
INERT = [-1e6, -1e6, 0, 0]
f32 = np.float32

# the vertex stage of these tests: the state's xy times viewSize (1, 1 where a test wants them unscaled: x * 1.0f is x), a colour
# whose first channel is the vertex's parity - 0 at a line's first vertex, 1 at its second -, alpha by the particle
PARITY = """struct FlowUniforms { float viewSize[2]; float time; float speedLimit; };
__device__ th_vertex th_vertex_main(const th_vertex_pass &v)
{
    const FlowUniforms &u = th_uniforms<FlowUniforms>(v);
    const float4 s = v.state;
    if (!(s.x != -1000000.0f || s.y != -1000000.0f)) return th_discard_vertex();
    th_vertex o;
    o.position = make_float2(s.x * u.viewSize[0], s.y * u.viewSize[1]);
    o.color = make_float4((float)(v.vertex & 1u), s.z, s.w, __builtin_fminf(__builtin_fmaxf(s.z * 40.0f + 0.5f, 0.125f), 0.875f));
    return o;
}
"""

# color.x - along: 0 wherever the varying is the library's own parameter; the second channel says so for the RGBA8 view too
ALONG_ZERO = """__device__ float4 th_fragment_main(const th_fragment_pass &f)
{
    const float d = f.color.x - th_line(f).along;
    return make_float4(d, d != 0.0f ? 1.0f : 0.0f, 1.0f, 1.0f);
}
"""

FIELDS = """__device__ float4 th_fragment_main(const th_fragment_pass &f)
{
    const th_fragment_line &l = th_line(f);
    return make_float4(l.along, l.across, l.length, f.color.w);
}
"""

LINE_ID = """__device__ float4 th_fragment_main(const th_fragment_pass &f)
{
    return make_float4((float)th_line(f).line, f.color.y, f.color.z, f.color.w);
}
"""


@pytest.fixture(scope="module")
def programs():
    from tendrils_amd.particles import DrawProgram, FragmentProgram
    made = dict(parity=DrawProgram.from_source(PARITY, FlowUniforms, "parity"),
                along_zero=FragmentProgram.from_source(ALONG_ZERO, name="along_zero"),
                fields=FragmentProgram.from_source(FIELDS, name="fields"),
                line_id=FragmentProgram.from_source(LINE_ID, name="line_id"),
                vignette=FragmentProgram.from_source(VIGNETTE, FragUniforms, "vignette"))
    yield made
    for p in made.values():
        p.dispose()


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def snap(p, n):
    """dep_snap (th_raster.hpp): rint(p * 8n + (8n - 8)) in fp32, two rounded operations"""
    return np.rint(p.astype(f32) * f32(8 * n) + f32(8 * n - 8)).astype(np.int64)


def to_f32(ints):
    """(float)integer: every integer here is below 2^53, so the double is exact and the fp32 is rounded once"""
    return np.array([float(v) for v in ints], np.float64).astype(f32)


def restate(keys, ends, view):
    """per fragment of `keys` (owner << 56 | texel << 32 | stream index): (line, along, across, length) as the issue defines them;
    ends: (ax, ay, bx, by) clip-space positions of every line's first and second vertex, by stream index"""
    fw, fh = view
    k = keys.astype(np.uint64)
    line = (k & np.uint64(0xffffffff)).astype(np.int64)
    texel = ((k >> np.uint64(32)) & np.uint64(0xffffff)).astype(np.int64)
    x, y = texel % fw, texel // fw
    ax, ay, bx, by = (e[line] for e in ends)
    sx0, sy0, sx1, sy1 = snap(ax, fw), snap(ay, fh), snap(bx, fw), snap(by, fh)
    num, den, crs = [], [], []
    for i in range(len(line)):                       # Python integers
        ex, ey = int(sx1[i]) - int(sx0[i]), int(sy1[i]) - int(sy0[i])
        qx, qy = 16 * int(x[i]) - int(sx0[i]), 16 * int(y[i]) - int(sy0[i])
        den.append(ex * ex + ey * ey)
        num.append(qx * ex + qy * ey)
        crs.append(qy * ex - qx * ey)
    numf, denf, crsf = to_f32(num), to_f32(den), to_f32(crs)
    flat = denf == 0
    safe = np.where(flat, f32(1), denf)
    len16 = np.sqrt(safe)
    along = np.where(flat, f32(0), numf / safe).astype(f32)
    across = np.where(flat, f32(0), (crsf / len16) * f32(0.0625)).astype(f32)
    length = np.where(flat, f32(0), len16 * f32(0.0625)).astype(f32)
    return line, along, across, length, np.array(den, dtype=object)


def fields_np(keys, colors, ends, view):
    _line, along, across, length, _den = restate(keys, ends, view)
    return np.stack([along, across, length, colors[:, 3]], 1).astype(f32)


def line_id_np(keys, colors, ends, view):
    out = colors.copy()
    out[:, 0] = (keys.astype(np.uint64) & np.uint64(0xffffffff)).astype(f32)
    return out


RESTATED = dict(fields=fields_np, line_id=line_id_np)


def by_stream(a):
    """[H, W] per particle -> per stream index (column * H + row)"""
    return np.ascontiguousarray(a.T).reshape(-1)


def stream_vertices(cur, prev):
    """The states the two vertices of every line read: vertex j of column i of the stream Particles.generateLUT([W, 2H]) through
    stateAtFrame (src/state/state-at-frame.glsl:12-22; th_stream.inc), in fp32 as the shader computes it.  For the shapes of these
    tests every vertex reads its line's own texel; WHICH buffer is the stream's to say: `previous` then `current` in the lower half
    of the rows, `current` twice above it (no line) and `current` then `previous` in the last row."""
    h, w = cur.shape[:2]
    inv_x, inv_y = 1.0 / (max(w, 2) - 1), 1.0 / (max(2 * h, 2) - 1)
    assert (tap_nearest((np.arange(w) * inv_x).astype(f32), w) == np.arange(w)).all()
    ends = []
    for odd in (0, 1):
        uvy = ((2 * np.arange(h) + odd) * inv_y).astype(f32)
        near = uvy * f32(h)
        fl = np.floor(near)
        assert (tap_nearest(fl / f32(h), h) == np.arange(h)).all()
        from_cur = (near - fl) > f32(0.25)
        ends.append(np.where(from_cur[:, None, None], cur, prev))
    return ends


def ends_of_state(cur, prev, view_size):
    """PARITY's positions, by stream index: the state's xy times viewSize"""
    vx, vy = f32(view_size[0]), f32(view_size[1])
    a, b = stream_vertices(cur, prev)
    return (by_stream(a[..., 0] * vx), by_stream(a[..., 1] * vy), by_stream(b[..., 0] * vx), by_stream(b[..., 1] * vy))


def ends_of_export(t, which, cur, prev):
    """the built-in stage's positions from th_export_lines / th_export_view_lines: the list is compacted in stream order, so its
    k-th line is the k-th stream index whose line exists (both vertices live, positions not equal)"""
    listed = t.export_lines(view=which == VIEW_PASS)
    ax, ay, bx, by = ends_of_state(cur, prev, t.viewSize)
    live = lambda s: by_stream((s[..., 0] != f32(-1e6)) | (s[..., 1] != f32(-1e6)))          # noqa: E731
    a, b = stream_vertices(cur, prev)
    exists = live(a) & live(b) & ~((ax == bx) & (ay == by))
    ids = np.flatnonzero(exists)
    assert len(ids) == len(listed) > 0
    ends = [np.zeros(cur.shape[0] * cur.shape[1], f32) for _ in range(4)]
    for e, column in zip(ends, range(4)):
        e[ids] = listed[:, column]
    assert bits_equal(ends[0][ids], ax[ids]).all() and bits_equal(ends[3][ids], by[ids]).all()        # (the pairing is what this test takes it for)
    return tuple(ends)


def emit_plain(t, which, vertex, u):
    """the EXISTING emit of the pass without a fragment stage"""
    from tendrils_amd import sharding
    if vertex is not None:
        return sharding.emit_program_fragments(t, vertex, which, u)
    return sharding.emit_view_fragments(t) if which == VIEW_PASS else sharding.emit_fragments(t)


def merge(t, which, keys, colors):
    from tendrils_amd import sharding
    (sharding.merge_view_fragments if which == VIEW_PASS else sharding.merge_fragments)(t, keys, colors)


def check_stage(programs, name, which, with_vertex, view, cur, prev, base, least=300, owners=1, ring=None, **made):
    """the stage `name` behind PARITY or the built-in vertex stage: th_draw_stages_emit's varyings against the restatement fragment
    by fragment, th_draw_stages_run's target against the restated fragments blended by the existing merge, emit + merge against
    the run.  ring: what a packed ring's texels decode to (the restatement's state); returns (keys, restated varyings)"""
    import torch
    from tendrils_amd import sharding
    got, em, ref = (make(view, cur, prev, base, color_map(), **made) for _ in range(3))
    rcur, rprev = ring if ring is not None else (cur, prev)
    vertex, u = (programs["parity"] if with_vertex else None), uniforms_of(got)
    n = stages_run(got, which, vertex, programs[name], u)
    assert last_draw(got) == (STREAM, n) and n >= least, (n, least)
    # the reference: the existing emit, the restatement, the existing merge
    ends = ends_of_state(rcur, rprev, got.viewSize) if with_vertex else ends_of_export(ref, which, rcur, rprev)
    keys, colors = emit_plain(ref, which, vertex, u)
    k = keys.cpu().numpy().astype(np.uint64)
    want = np.ascontiguousarray(RESTATED[name](k, colors.cpu().numpy(), ends, view), f32)
    assert len(k) == n
    # the emit: the stage's own output against the restatement, fragment by fragment
    sharding.set_owners(em, owners)
    ekeys, ecolors = sharding.emit_stage_fragments(em, vertex, programs[name], which, u)
    ek, ec = ekeys.cpu().numpy().astype(np.uint64), ecolors.cpu().numpy()
    assert len(ek) == n and last_draw(em) == (STREAM, n)
    assert set((ek >> np.uint64(56)).tolist()) == set(range(owners))
    low = np.uint64(0x00ffffffffffffff)
    order = np.argsort(ek & low, kind="stable")      # (parted by owner: back to texel, stream index)
    order_ref = np.argsort(k & low, kind="stable")
    assert (ek[order] & low == k[order_ref] & low).all()
    differ = ~bits_equal(ec[order], want[order_ref])
    wrong = differ.any(axis=1)
    assert not wrong.any(), (name, which, with_vertex, "fragments", int(wrong.sum()), "by channel", differ.sum(axis=0).tolist(),
                             [hex(v) for v in k[order_ref][wrong][:4]], ec[order][wrong][:4], want[order_ref][wrong][:4])
    # the run against the restated fragments blended by the existing merge, then the emit's own merge against the run
    merge(ref, which, keys.clone(), torch.from_numpy(want).cuda().contiguous())
    assert same(target(got, which), target(ref, which)), (name, which, with_vertex, "the run against the restatement")
    merge(em, which, ekeys, ecolors)
    assert same(target(em, which), target(got, which)), (name, which, with_vertex, "emit + merge against the run")
    for b in range(2):                               # the ring is untouched
        assert bits_equal(got.particles.read(b), (rcur, rprev)[b]).all()
    for t in (got, em, ref):
        t.dispose()
    return k, want


# ---- 1. `along` is the library's own parameter -----------------------------------------------------------------------------------------
def wide(t, width):
    """a GL that honours gl.lineWidth: both passes at `width` (the context was made with a range that lets it through)"""
    t.state["flowWidth"] = t.state["lineWidth"] = width
    t.line_widths()
    return t


def along_cases():
    yield "hashed", (97, 61), deposit_hashed_inputs(48, 11, 1.05, 0.08, 11), {}
    for fixture in ("deposit_long_lines_32", "deposit_border_48"):
        fx = load(os.path.join(GOLDEN, fixture + ".npz"))
        m = fx["meta"]
        yield fixture, tuple(m["viewRes"]), (fx["current"], fx["previous"]), dict(time=m["time"], view_size=m["viewSize"], speed_limit=m["speedLimit"])


@pytest.mark.parametrize("width", [1, 5])
@pytest.mark.parametrize("case", ["hashed", "deposit_long_lines_32", "deposit_border_48"])
def test_along_is_the_parameter_the_varying_was_mixed_with(programs, case, width):
    name, view, (cur, prev), made = next(c for c in along_cases() if c[0] == case)
    base = base_flow(view, 12)
    assert (base[..., 0] != 0).all()                 # (a texel no line touched keeps a first channel that is not 0)
    for which in (FLOW_PASS, VIEW_PASS):
        got = wide(make(view, cur, prev, base, color_map(), lineWidthRange=(1, 8), **made), width)
        ref = wide(make(view, cur, prev, base, color_map(), lineWidthRange=(1, 8), **made), width)
        u = uniforms_of(got)
        n = stages_run(got, which, programs["parity"], programs["along_zero"], u)
        keys, _colors = emit_plain(ref, which, programs["parity"], u)            # which texels the lines touch: the existing emit
        texel = ((keys.cpu().numpy().astype(np.uint64) >> np.uint64(32)) & np.uint64(0xffffff)).astype(np.int64)
        assert n == len(texel) >= (1000 if case != "hashed" else 300)
        touched = np.zeros(view[0] * view[1], bool)
        touched[texel] = True
        touched = touched.reshape(view[1], view[0])
        assert touched.any() and not touched.all()
        drawn = target(got, which)
        if which == FLOW_PASS:
            assert (drawn[touched] == np.array([0, 0, 1, 1], f32)).all(), drawn[touched][(drawn[touched] != np.array([0, 0, 1, 1], f32)).any(axis=1)][:4]
            assert bits_equal(drawn[~touched], base[~touched]).all()
        else:
            assert (drawn[touched] == np.array([0, 0, 255, 255], np.uint8)).all() and not drawn[~touched].any()
        got.dispose()
        ref.dispose()


# ---- 2. line, across, length against numpy: a vertex program that passes the state's xy through ------------------------------------
def with_special_lines(cur, prev, view):
    """... a line whose endpoints differ and snap to one point - the centre of a texel: clip-space 0 on a target of odd extent,
    1 / width on an even one (all heights here are odd); 1e-6 of clip space is far less than 1/16 texel -, and two lines with an
    inert end, which draw nothing"""
    cur, prev = cur.copy(), prev.copy()
    assert view[1] & 1
    x0 = 0.0 if view[0] & 1 else 1.0 / view[0]
    prev[0, 0] = [x0, 0.0, 0.004, -0.003]
    cur[0, 0] = [x0 + 1e-6, 0.0, 0.004, -0.003]
    prev[1, 1] = INERT
    cur[1, 1] = [0.2, 0.1, 0.001, 0.002]
    prev[2, 1] = [0.25, -0.1, 0.001, 0.002]
    cur[2, 1] = INERT
    return cur, prev


def xy_cases(case):
    if case == "33x17":
        return (33, 17), with_special_lines(*deposit_hashed_inputs(32, 21, 0.95, 0.07, 11), (33, 17)), 300
    if case == "97x61":
        return (97, 61), with_special_lines(*deposit_hashed_inputs(48, 23, 1.05, 0.08, 11), (97, 61)), 300
    # 1100 x 3: a line of about 1078 texels - more than 2^14 sixteenths between its snapped endpoints: dep_param's 64-bit branch
    cur, prev = with_special_lines(*deposit_hashed_inputs(8, 25, 0.9, 0.01, 0), (1100, 3))
    prev[3, 2] = [-0.98, -0.2, 0.002, 0.001]
    cur[3, 2] = [0.98, 0.3, 0.002, 0.001]
    return (1100, 3), (cur, prev), 1000


@pytest.mark.parametrize("case", ["33x17", "97x61", "1100x3"])
def test_line_across_and_length_equal_their_restatement(programs, case):
    view, (cur, prev), least = xy_cases(case)
    for which in (FLOW_PASS, VIEW_PASS):
        k, want = check_stage(programs, "fields", which, True, view, cur, prev, base_flow(view, 22), least=least, view_size=(1.0, 1.0))
        check_stage(programs, "line_id", which, True, view, cur, prev, base_flow(view, 22), least=least, view_size=(1.0, 1.0))
        if which == VIEW_PASS:
            continue
        # the inputs are what they are meant to be
        line, _along, _across, length, den = restate(k, ends_of_state(cur, prev, (1.0, 1.0)), view)
        flat = np.array([d == 0 for d in den])
        assert (line == 0).any() and flat[line == 0].all()                      # particle (row 0, column 0): stream index 0
        assert not want[flat][:, :3].any()
        n = cur.shape[0]
        assert not np.isin(line, [1 * n + 1, 1 * n + 2]).any()                  # the lines with an inert end drew nothing
        assert (want[~flat][:, 2] > 0).all() and (want[:, 1] < 0).any() and (want[:, 1] > 0).any()
        if case == "1100x3":
            long_line = line == 2 * n + 3
            assert long_line.sum() > 1000 and float(length[long_line][0]) > 1024.0
            assert max(den[long_line]) > (1 << 28)


# ---- 3. the built-in vertex stage ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fields", "line_id"])
def test_the_builtin_vertex_stage(programs, name):
    n, view = 48, (97, 61)
    cur, prev = with_special_lines(*deposit_hashed_inputs(n, 31, 1.05, 0.08, 11), view)
    for which in (FLOW_PASS, VIEW_PASS):
        check_stage(programs, name, which, False, view, cur, prev, base_flow(view, 32))


def test_a_packed_ring_draws_what_its_texels_decode_to(programs):
    n, view = 48, (97, 61)
    cur, prev = deposit_hashed_inputs(n, 33, 1.05, 0.08, 11)
    base = base_flow(view, 34)
    for which in (FLOW_PASS, VIEW_PASS):
        for with_vertex in (False, True):
            packed = make(view, cur, prev, base, color_map(), fmt="f16")
            decoded = packed.particles.read(0), packed.particles.read(1)
            plain = make(view, decoded[0], decoded[1], base, color_map())
            vertex, u = (programs["parity"] if with_vertex else None), uniforms_of(plain)
            want_n = stages_run(plain, which, vertex, programs["fields"], u)
            assert stages_run(packed, which, vertex, programs["fields"], u) == want_n > 300
            assert same(target(packed, which), target(plain, which))
            assert sorted_buffers(packed) == 0
            for b in range(2):
                assert bits_equal(packed.particles.read(b), decoded[b]).all()
            packed.dispose()
            plain.dispose()
    check_stage(programs, "fields", FLOW_PASS, False, view, cur, prev, base, fmt="f16", ring=decoded)


def test_a_tile_sorted_ring_goes_to_texel_order_and_draws_the_same_bits(programs):
    n, view = 48, (33, 31)                         # (slots are sorted only where the texture has twice the field's texels)
    st = np.zeros((n, n, 4), f32)
    rng = np.random.default_rng(35)
    st[..., :2] = rng.uniform(-.9, .9, (n, n, 2))
    st[..., 2:] = rng.uniform(-.008, .008, (n, n, 2))

    def looped():
        """built-in steps and binned draws: the ring lies in tile-sorted slots"""
        t = make(view, st, st, np.zeros((view[1], view[0], 4), f32), color_map())
        assert t.particles.option("bucket", 1) == 1
        t.particles.draw_pipeline("bins")
        t.timer.time = 1000.0
        for k in range(3):
            t.timer.tick()
            t.step()
            if k < 2:
                t.draw()
        return t

    for which in (FLOW_PASS, VIEW_PASS):
        held, read = looped(), looped()
        assert sorted_buffers(held) > 0
        ring = read.particles.read(0), read.particles.read(1)          # (reading takes `read` to texel order)
        assert sorted_buffers(read) == 0 and sorted_buffers(held) > 0
        u = uniforms_of(held)
        want_n = stages_run(read, which, None, programs["fields"], u)
        assert stages_run(held, which, None, programs["fields"], u) == want_n > 300
        assert last_draw(held) == (STREAM, want_n)
        assert sorted_buffers(held) == 0                                # afterwards the ring is in texel order
        assert same(target(held, which), target(read, which))
        for b in range(2):
            assert bits_equal(held.particles.read(b), ring[b]).all()
        held.dispose()
        read.dispose()


# ---- 4. emit + merge at several owners ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("owners", [1, 3])
def test_emit_and_merge_equal_the_run_and_line_is_the_keys_low_word(programs, owners):
    n, view = 48, (97, 61)
    cur, prev = deposit_hashed_inputs(n, 41, 1.05, 0.08, 11)
    for which in (FLOW_PASS, VIEW_PASS):
        for with_vertex in (False, True):
            # (check_stage: the emitted varyings' first channel against (float)(key & 0xffffffff), fragment by fragment)
            check_stage(programs, "line_id", which, with_vertex, view, cur, prev, base_flow(view, 42), owners=owners)
    check_stage(programs, "fields", FLOW_PASS, True, view, cur, prev, base_flow(view, 42), owners=owners)


@pytest.mark.parametrize("name", ["line_id", "fields"])
def test_two_row_bands_emit_what_the_whole_texture_runs(programs, name):
    """bands of 20 and 28 rows (the second starts at row 20: row0 is not 0): `line` is the GLOBAL stream index, the geometry the
    whole target's - both bands' emits in one merge leave what th_draw_stages_run of the whole texture leaves"""
    import torch
    from tendrils_amd import sharding
    n, view = 48, (97, 61)
    cur, prev = deposit_hashed_inputs(n, 43, 1.05, 0.08, 11)
    base = base_flow(view, 44)
    for which in (FLOW_PASS, VIEW_PASS):
        for with_vertex in (False, True):
            run, owner = make(view, cur, prev, base, color_map()), make(view, cur, prev, base, color_map())
            bands = [make(view, cur, prev, base, color_map(), band=b) for b in ((0, 20), (20, 28))]
            vertex, u = (programs["parity"] if with_vertex else None), uniforms_of(run)
            want_n = stages_run(run, which, vertex, programs[name], u)
            parts = []
            for t, (row0, rows) in zip(bands, ((0, 20), (20, 28))):
                keys, colors = sharding.emit_stage_fragments(t, vertex, programs[name], which, u)
                k, c = keys.cpu().numpy().astype(np.uint64), colors.cpu().numpy()
                line = (k & np.uint64(0xffffffff)).astype(np.int64)
                assert len(k) > 100 and (line % n >= row0).all() and (line % n < row0 + rows).all()
                if name == "line_id":
                    assert (c[:, 0] == line.astype(f32)).all()
                parts.append((keys.clone(), colors.clone()))
            keys, colors = torch.cat([p[0] for p in parts]).contiguous(), torch.cat([p[1] for p in parts]).contiguous()
            assert int(keys.numel()) == want_n > 300
            merge(owner, which, keys, colors)
            assert same(target(owner, which), target(run, which)), (name, which, with_vertex)
            for t in [run, owner] + bands:
                t.dispose()


# ---- 5. routing ------------------------------------------------------------------------------------------------------------------------
def test_a_stage_that_reads_the_line_stays_stream_ordered_under_stage_bins(programs):
    from tendrils_amd import _capi
    n, view = 48, (97, 61)
    cur, prev = deposit_hashed_inputs(n, 51, 1.05, 0.08, 11)
    base = base_flow(view, 52)
    for which in (FLOW_PASS, VIEW_PASS):
        for with_vertex in (False, True):
            on, off = make(view, cur, prev, base, color_map()), make(view, cur, prev, base, color_map())
            for t, option in ((on, 1), (off, 0)):
                t.particles.draw_pipeline("bins")
                assert t.particles.option("stage_bins", option) == option
            vertex, u = (programs["parity"] if with_vertex else None), uniforms_of(on)
            n_on = stages_run(on, which, vertex, programs["fields"], u)
            assert last_draw(on) == (STREAM, n_on)
            n_off = stages_run(off, which, vertex, programs["fields"], u)
            assert last_draw(off) == (STREAM, n_off) and n_on == n_off > 300
            assert same(target(on, which), target(off, which))
            # VIGNETTE in the same contexts: through the bins with the option, stream-ordered without - and one fragment launch
            for t, pipeline in ((on, BINS), (off, STREAM)):
                t.flow.set_pixels(base)
                t.clearView()
                _capi.call("th_kernel_timing", t.particles._ctx, 1)
                assert stages_run(t, which, None, programs["vignette"], u) == n_on
                assert last_draw(t) == (pipeline, n_on)
                assert kernel_launches(t) == 1
            assert same(target(on, which), target(off, which))
            # ... and a pass that reads the line brackets one launch too: the stage's (the line kernel is the raster's side)
            assert stages_run(off, which, None, programs["fields"], u) == n_on
            assert kernel_launches(off) == 1
            on.dispose()
            off.dispose()


# ---- 6. nothing to draw, and what is refused ---------------------------------------------------------------------------------------------
def test_an_all_inert_state_launches_nothing(programs):
    from tendrils_amd import _capi, sharding
    n, view = 32, (64, 64)
    inert = np.tile(np.array(INERT, f32), (n, n, 1))
    base = base_flow(view, 61)
    t = make(view, inert, inert, base, color_map())
    _capi.call("th_kernel_timing", t.particles._ctx, 1)
    before = t.read_view()
    for vertex, launches in ((None, 0), (programs["parity"], 4)):          # (the event pairs sit around a vertex program's kernel too: four passes)
        for which in (FLOW_PASS, VIEW_PASS):
            assert stages_run(t, which, vertex, programs["fields"], uniforms_of(t)) == 0
            assert last_draw(t) == (STREAM, 0)
            keys, _colors = sharding.emit_stage_fragments(t, vertex, programs["fields"], which, uniforms_of(t))
            assert keys.numel() == 0
        assert kernel_launches(t) == launches
    assert bits_equal(t.flow.read(), base).all() and (t.read_view() == before).all()
    t.dispose()


def test_refusals_are_unchanged_with_such_a_program_in_the_slot(programs):
    from tendrils_amd import _capi
    lib = _capi.load()
    n, view = 32, (64, 64)
    cur, prev = deposit_hashed_inputs(n, 71, 1.0, 0.05, 0)
    base = base_flow(view, 72)
    t = make(view, cur, prev, base, color_map())
    u = uniforms_of(t)
    view_before = t.read_view()
    frag, vert = programs["fields"], programs["parity"]
    vblock = vert.pack(u)
    big = (C.c_uint8 * 1025)()
    some = (C.c_uint8 * 16)()
    d = t.deposit_uniforms()

    def stages(vertex=None, vu=None, vn=0, fragment=None, fu=None, fn=0, builtin=None):
        s = _capi.DrawStages()
        s.vertex, s.fragment = (vertex.handle if vertex else None), (fragment.handle if fragment else None)
        s.vertex_uniforms = C.cast(C.pointer(vu), C.c_void_p) if vu is not None else None
        s.fragment_uniforms = C.cast(C.pointer(fu), C.c_void_p) if fu is not None else None
        s.vertex_uniform_bytes, s.fragment_uniform_bytes = vn, fn
        s.builtin = C.cast(C.pointer(builtin), C.c_void_p) if builtin is not None else None
        return s

    vsize = C.sizeof(vblock)
    cases = [("a fragment program as the vertex stage", stages(vertex=frag), FLOW_PASS, ["draw program", "fragment program"]),
             ("a draw program as the fragment stage", stages(fragment=vert, fu=vblock, fn=vsize, builtin=d), FLOW_PASS, ["draw program", "fragment program"]),
             ("1025 fragment uniform bytes", stages(fragment=frag, fu=big, fn=1025, builtin=d), FLOW_PASS, ["1025"]),
             ("null fragment uniforms with a size", stages(fragment=frag, fn=16, builtin=d), FLOW_PASS, ["null"]),
             ("no vertex program and no builtin", stages(fragment=frag, fu=some, fn=16), FLOW_PASS, ["builtin"]),
             ("an unknown pass", stages(fragment=frag, builtin=d), 2, ["pass 2"])]
    for what, s, which, words in cases:
        count, kp, cp = C.c_uint64(7), C.c_void_p(), C.c_void_p()
        for status in (lib.th_draw_stages_run(t.particles._ctx, C.byref(s), which, C.byref(count)),
                       lib.th_draw_stages_emit(t.particles._ctx, C.byref(s), which, C.byref(count), C.byref(kp), C.byref(cp))):
            assert status == _capi.TH_ERR_INVALID, what
            message = lib.th_last_error().decode()
            assert all(w in message for w in words), (what, message)
        assert not kp.value and not cp.value
        assert bits_equal(t.flow.read(), base).all() and (t.read_view() == view_before).all(), what
    ok = stages(fragment=frag, builtin=d)
    assert lib.th_draw_stages_emit(t.particles._ctx, C.byref(ok), FLOW_PASS, None, None, None) == _capi.TH_ERR_INVALID      # null outputs
    n_out = C.c_uint64(0)
    assert lib.th_draw_program_run(t.particles._ctx, frag.handle, None, 0, FLOW_PASS, C.byref(n_out)) == _capi.TH_ERR_INVALID
    assert b"fragment program" in lib.th_last_error() and b"draw program" in lib.th_last_error()
    assert bits_equal(t.flow.read(), base).all() and (t.read_view() == view_before).all()
    # th_program_query serves it as it serves the others: th_fragment_kernel, no scratch, no LDS
    q = frag.query(t.particles)
    assert q["scratch_bytes"] == 0 and q["lds_bytes"] == 0 and q["code_bytes"] > 0, q
    t.dispose()
    # a row band: the local run is refused, nothing launched
    band = make(view, cur, prev, base, color_map(), band=(0, 16))
    s = stages(fragment=frag, builtin=d)
    assert lib.th_draw_stages_run(band.particles._ctx, C.byref(s), FLOW_PASS, C.byref(n_out)) == _capi.TH_ERR_UNSUPPORTED
    assert b"th_draw_stages_emit" in lib.th_last_error()
    assert bits_equal(band.flow.read(), base).all()
    band.dispose()
