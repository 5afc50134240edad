"""Draw programs on the GPU (include/tendrils_hip.h "draw programs"; tendrils_amd/csrc/th_drawprog.hip and th_draw_prelude.inc): a
caller's vertex stage in the passes of draw().  Everything is compared on the bits: the library's own stages written out as
programs must leave what th_flow_deposit / th_view_draw leave, other stages what the restatement leaves on inputs transformed
exactly; the ring is untouched, nothing is reused across a program pass, the entry points refuse each other's programs."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import bits_equal, golden, load
from test_deposit_oracle import deposit_inputs
from test_draw_program_build import FLOW
from test_program_build import DRIFT
from test_screen_program_build import COPY

pytestmark = pytest.mark.gpu

INERT = [-1e6, -1e6, 0, 0]

# the flow stage seen in a mirror: x and the x velocity negated (exact in fp32)
MIRROR = """struct FlowUniforms { float viewSize[2]; float time; float speedLimit; };
__device__ th_vertex th_vertex_main(const th_vertex_pass &v)
{
    const FlowUniforms &u = th_uniforms<FlowUniforms>(v);
    const float4 s = v.state;
    if (!(s.x != -1000000.0f || s.y != -1000000.0f)) return th_discard_vertex();
    th_vertex o;
    o.position = make_float2(-s.x * u.viewSize[0], s.y * u.viewSize[1]);
    o.color = make_float4(-s.z, s.w, u.time, __builtin_fminf(__builtin_sqrtf(s.z * s.z + s.w * s.w) / u.speedLimit, 1.0f));
    return o;
}
"""

# ... zoomed: a uniform multiplies the position
ZOOM = """struct ZoomUniforms { float viewSize[2]; float time; float speedLimit; float zoom; };
__device__ th_vertex th_vertex_main(const th_vertex_pass &v)
{
    const ZoomUniforms &u = th_uniforms<ZoomUniforms>(v);
    const float4 s = v.state;
    if (!(s.x != -1000000.0f || s.y != -1000000.0f)) return th_discard_vertex();
    th_vertex o;
    o.position = make_float2(s.x * u.viewSize[0] * u.zoom, s.y * u.viewSize[1] * u.zoom);
    o.color = make_float4(s.z, s.w, u.time, __builtin_fminf(__builtin_sqrtf(s.z * s.z + s.w * s.w) / u.speedLimit, 1.0f));
    return o;
}
"""

# ... of the lines of even stream index alone
EVEN_LINES = FLOW.replace("    const float4 s = v.state;\n", "    const float4 s = v.state;\n    if (v.line & 1u) return th_discard_vertex();\n")

# the library's own view stage, written out as a program (tendrils_amd/csrc/th_raster.hpp: dep_render_color)
VIEW = """struct ViewUniforms { float viewSize[2]; float time, speedLimit, flowDecay, speedAlpha, colorMapAlpha, sinTerm; float baseColor[4], flowColor[4]; };
__device__ th_vertex th_vertex_main(const th_vertex_pass &v)
{
    const ViewUniforms &u = th_uniforms<ViewUniforms>(v);
    const float4 state = v.state;
    if (!(state.x != -1000000.0f || state.y != -1000000.0f)) return th_discard_vertex();
    const float velx = state.z / u.speedLimit, vely = state.w / u.speedLimit;
    const float speed_rate = __builtin_fminf((velx * velx + vely * vely) / u.speedAlpha, 1.0f);
    const float4 m = th_colormap(v, v.uv.x * v.geomRes.x / v.dataRes.x, v.uv.y * v.geomRes.y / v.dataRes.y);
    float mapped[4] = {m.x, m.y, m.z, m.w};
    for (int k = 0; k < 4; ++k) mapped[k] = mapped[k] * u.colorMapAlpha;
    const float al[3] = {velx * 1.0f + vely * 0.0f, velx * -0.5000000000000004f + vely * -0.8660254037844385f,
                         velx * -0.4999999999999998f + vely * 0.8660254037844387f};
    const float gbr[3] = {al[1] * (1.0f - u.flowDecay), al[2] * (1.0f - u.flowDecay), al[0] * (1.0f - u.flowDecay)};
    float flw[4];
    for (int k = 0; k < 3; ++k) {
        const float mixed = al[k] * (1.0f - u.sinTerm) + gbr[k] * u.sinTerm;
        flw[k] = u.flowColor[k] * (0.0f + (1.0f - 0.0f) * (mixed - -1.0f) / (1.0f - -1.0f));
    }
    flw[3] = u.flowColor[3];
    float c[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    auto add = [&](const float *t) {
        const float a = t[3];
        const float pre[4] = {t[0] * a, t[1] * a, t[2] * a, a};
        for (int k = 0; k < 4; ++k) c[k] = c[k] + __builtin_fminf(__builtin_fmaxf(pre[k], 0.0f), 1.0f);
    };
    add(u.baseColor); add(mapped); add(flw);
    const float amount = __builtin_fminf(1.0f - (__builtin_sqrtf(state.x * state.x + state.y * state.y) / 1.0f), 1.0f);
    const float ut = 1.0f - amount;
    const float bz = (0.2f * ut + 1.0f * amount) * ut + (1.0f * ut + 1.0f * amount) * amount;
    const float vg = __builtin_fmaxf(0.0f, bz);
    c[3] = c[3] * (speed_rate * __builtin_fminf(__builtin_fmaxf(vg, 0.2f), 1.0f));
    th_vertex o;
    o.position = make_float2(state.x * u.viewSize[0], state.y * u.viewSize[1]);
    o.color = make_float4(c[0], c[1], c[2], c[3]);
    return o;
}
"""

POSITION = """    const FlowUniforms &u = th_uniforms<FlowUniforms>(v);
    const float4 s = v.state;
    if (!(s.x != -1000000.0f || s.y != -1000000.0f)) return th_discard_vertex();
    th_vertex o;
    o.position = make_float2(s.x * u.viewSize[0], s.y * u.viewSize[1]);
"""
# the colour is the flow field at the vertex's own position
TAP_FLOW = """struct FlowUniforms { float viewSize[2]; float time; float speedLimit; };
__device__ th_vertex th_vertex_main(const th_vertex_pass &v)
{
""" + POSITION + """    o.color = th_flow(v, o.position.x * 0.5f + 0.5f, o.position.y * 0.5f + 0.5f);
    return o;
}
"""
# ... texel (column, vertex) of a colour map of the stream's shape
FROM_MAP = """struct FlowUniforms { float viewSize[2]; float time; float speedLimit; };
__device__ th_vertex th_vertex_main(const th_vertex_pass &v)
{
""" + POSITION + """    o.color = th_colormap(v, ((float)v.column + 0.5f) / v.geomRes.x, ((float)v.vertex + 0.5f) / v.geomRes.y);
    return o;
}
"""
# ... the shapes the accessors report and a tap of the colour map, opaque: a covered texel holds exactly this colour
SHAPES = """struct FlowUniforms { float viewSize[2]; float time; float speedLimit; };
__device__ th_vertex th_vertex_main(const th_vertex_pass &v)
{
""" + POSITION + """    const float2 f = th_flow_res(v), c = th_colormap_res(v);
    const float4 m = th_colormap(v, 0.3f, 0.7f);
    o.color = make_float4(f.x * 1024.0f + f.y, c.x * 1024.0f + c.y, ((m.x + m.y) + m.z) + m.w, 1.0f);
    return o;
}
"""


class FlowUniforms(C.Structure):
    _fields_ = [("viewSize", C.c_float * 2), ("time", C.c_float), ("speedLimit", C.c_float)]


class ZoomUniforms(C.Structure):
    _fields_ = FlowUniforms._fields_ + [("zoom", C.c_float)]


class ViewUniforms(C.Structure):
    _fields_ = [("viewSize", C.c_float * 2), ("time", C.c_float), ("speedLimit", C.c_float), ("flowDecay", C.c_float),
                ("speedAlpha", C.c_float), ("colorMapAlpha", C.c_float), ("sinTerm", C.c_float),
                ("baseColor", C.c_float * 4), ("flowColor", C.c_float * 4)]


class Padded(C.Structure):                   # a block of exactly 1024 bytes that begins as FlowUniforms does
    _fields_ = FlowUniforms._fields_ + [("rest", C.c_uint8 * (1024 - C.sizeof(FlowUniforms)))]


@pytest.fixture(scope="module")
def programs():
    """every program of this module, compiled once"""
    from tendrils_amd.particles import DrawProgram, Program, ScreenProgram
    made = dict(flow=DrawProgram.from_source(FLOW, FlowUniforms, "flow_stage"),
                view=DrawProgram.from_source(VIEW, ViewUniforms, "view_stage"),
                mirror=DrawProgram.from_source(MIRROR, FlowUniforms, "mirror"),
                zoom=DrawProgram.from_source(ZOOM, ZoomUniforms, "zoom"),
                even=DrawProgram.from_source(EVEN_LINES, FlowUniforms, "even_lines"),
                tap=DrawProgram.from_source(TAP_FLOW, FlowUniforms, "tap_flow"),
                from_map=DrawProgram.from_source(FROM_MAP, FlowUniforms, "from_map"),
                shapes=DrawProgram.from_source(SHAPES, FlowUniforms, "shapes"),
                padded=DrawProgram.from_source(FLOW, Padded, "flow_stage_padded"),
                state=Program.from_source(DRIFT, name="drift"),
                screen=ScreenProgram.from_source(COPY, name="copy"))
    yield made
    for p in made.values():
        p.dispose()


def make(n, view_res, view_size=None, speed_limit=None, **options):
    import tendrils_amd as ta
    from tendrils_amd.tendrils import View
    opts = ta.defaults()
    opts.update(options)
    t = ta.Tendrils(View(*view_res), opts)
    t.resize()
    t.setup(n)
    if view_size is not None:
        t.viewSize[:] = view_size
    if speed_limit is not None:
        t.state["speedLimit"] = speed_limit
    return t


def flow_pass(cur, prev, base, time, view_res, view_size=None, speed_limit=None, program=None, prepare=None, render=None, **options):
    """the flow pass of draw() on a fresh context - with `program` as its vertex stage, else the library's own -: (flow, fragments)"""
    t = make(cur.shape[0], view_res, view_size, speed_limit, renderView=False, flowShader=program, **options)
    if prepare:
        prepare(t)
    t.uniforms["render"].update(render or {})
    t.particles.upload_texels(cur, 0)
    t.particles.upload_texels(prev, 1)
    t.flow.set_pixels(base)
    t.timer.time = time
    t.draw()
    got, frags = t.flow.read(), t.fragments
    t.dispose()
    return got, frags


def random_lines(n, seed, spread=1.2, step=.05, inert=0.1, aspect=1.0):
    rng = np.random.default_rng(seed)
    prev = np.zeros((n, n, 4), np.float32)
    prev[..., :2] = rng.uniform(-spread, spread, (n, n, 2)) * [1.0, aspect]
    prev[..., 2:] = rng.uniform(-.012, .012, (n, n, 2))
    cur = prev.copy()
    cur[..., :2] += rng.uniform(-step, step, (n, n, 2)).astype(np.float32)
    cur[..., 2:] = rng.uniform(-.012, .012, (n, n, 2))
    if inert:
        cur[rng.random((n, n)) < inert] = INERT
    return cur, prev


def live(st):
    return ~((st[..., 0] == np.float32(-1e6)) & (st[..., 1] == np.float32(-1e6)))


# ---- 1. the flow stage written out as a program is the library's ----------------------------------------------------------------
@pytest.mark.parametrize("path", golden("deposit"), ids=lambda p: p.split("/")[-1][:-4])
def test_restated_flow_stage_equals_the_library_and_the_oracle(oracle, programs, path):
    fx = load(path)
    m, base, _ = deposit_inputs(fx)
    args = (fx["current"], fx["previous"], base, m["time"], m["viewRes"], m["viewSize"], m["speedLimit"])
    got, frags = flow_pass(*args, program=programs["flow"])
    lib, lib_frags = flow_pass(*args)
    want, n = oracle.flow_deposit(fx["current"], fx["previous"], base, m["time"], view_size=m["viewSize"], speedLimit=m["speedLimit"])
    assert frags == lib_frags == n and n > 0
    assert bits_equal(got, lib).all()
    assert bits_equal(got, want).all()


def test_restated_flow_stage_where_the_lookups_drift(programs):
    """n = 100: some rows' vertices are other particles' texels - the program sees the texel and the buffer dep_fetch selects"""
    cur, prev = random_lines(100, 6)
    base = np.zeros((54, 96, 4), np.float32)
    got, frags = flow_pass(cur, prev, base, 321.0, (96, 54), program=programs["flow"])
    want, n = flow_pass(cur, prev, base, 321.0, (96, 54), prepare=lambda t: t.particles.draw_pipeline("stream"))
    assert frags == n and n > 3000
    assert bits_equal(got, want).all()


# ---- 2. the view stage written out as a program is th_view_draw -----------------------------------------------------------------
def view_frame(program, cur, prev, cmap, time):
    n, view = cur.shape[0], (96, 54)
    t = make(n, view, renderShader=program)
    t.state.update(speedAlpha=0.5, fadeColor=[0.1333, 0.1333, 0.1333, 0.3], baseColor=[1, 0.6, 0.2, 0.5], flowColor=[0.3, 1, 0.8, 0.4])
    t.colorMap.set_pixels(cmap)
    t.particles.upload_texels(cur, 0)
    t.particles.upload_texels(prev, 1)
    t.timer.time = time
    t.drawFill([0.9, 0.2, 0.4, 0.7])              # something under the fade and the lines
    t.uniforms["render"]["sinTerm"] = t.render_uniforms().sinTerm
    t.draw()
    out = t.read_view(), t.flow.read(), t.view_fragments
    t.dispose()
    return out


def test_restated_view_stage_equals_th_view_draw(programs):
    cur, prev = random_lines(64, 15, spread=0.9, step=.08, inert=0.03, aspect=54 / 96)
    cmap = np.random.default_rng(16).uniform(0, 1, (11, 13, 4)).astype(np.float32)
    got, got_flow, frags = view_frame(programs["view"], cur, prev, cmap, 1016.5)
    want, want_flow, n = view_frame(None, cur, prev, cmap, 1016.5)
    assert frags == n and n > 3000
    assert (got == want).all() and len(np.unique(want.reshape(-1, 4), axis=0)) > 100
    assert bits_equal(got_flow, want_flow).all()


# ---- 3. stages that are not the library's, against the restatement on inputs transformed exactly -------------------------------
def test_mirrored_stage_equals_the_oracle_on_mirrored_states(oracle, programs):
    cur, prev = random_lines(64, 31, spread=1.1, aspect=54 / 96)
    base = np.zeros((54, 96, 4), np.float32)
    got, frags = flow_pass(cur, prev, base, 700.0, (96, 54), program=programs["mirror"])
    flipped = []
    for st in (cur, prev):
        f = st.copy()
        f[..., 0] = np.where(live(st), -st[..., 0], st[..., 0])
        f[..., 2] = np.where(live(st), -st[..., 2], st[..., 2])
        flipped.append(f)
    want, n = oracle.flow_deposit(flipped[0], flipped[1], base, 700.0, view_size=(1.0, 96 / 54))
    plain, _ = oracle.flow_deposit(cur, prev, base, 700.0, view_size=(1.0, 96 / 54))
    assert frags == n and n > 1000
    assert bits_equal(got, want).all() and not bits_equal(got, plain).all()


def test_zoomed_stage_equals_the_restatement_on_halved_positions(oracle, programs):
    cur, prev = random_lines(64, 32, spread=1.6, aspect=54 / 96)
    base = np.zeros((54, 96, 4), np.float32)
    got, frags = flow_pass(cur, prev, base, 700.0, (96, 54), program=programs["zoom"], render=dict(zoom=0.5))
    halved = []
    for st in (cur, prev):
        h = st.copy()
        h[..., :2] = np.where(live(st)[..., None], st[..., :2] * np.float32(0.5), st[..., :2])
        halved.append(h)
    want, n = oracle.flow_deposit(halved[0], halved[1], base, 700.0, view_size=(1.0, 96 / 54))
    assert frags == n and n > 1000
    assert bits_equal(got, want).all()


def test_discarded_lines_equal_the_restatement_with_those_particles_inert(oracle, programs):
    n = 64                                          # (no lookup drifts: a line's vertices are its own particle's texels)
    cur, prev = random_lines(n, 33, spread=1.0, aspect=54 / 96)
    base = np.zeros((54, 96, 4), np.float32)
    got, frags = flow_pass(cur, prev, base, 700.0, (96, 54), program=programs["even"])
    row, col = np.mgrid[0:n, 0:n]
    odd = ((col * n + row) & 1).astype(bool)       # the stream index of particle (row, col)'s line
    cur2, prev2 = cur.copy(), prev.copy()
    cur2[odd] = INERT
    prev2[odd] = INERT
    want, count = oracle.flow_deposit(cur2, prev2, base, 700.0, view_size=(1.0, 96 / 54))
    assert frags == count and 500 < count
    assert bits_equal(got, want).all()


# ---- 4. crowded texels ----------------------------------------------------------------------------------------------------------
def test_crowded_texels_are_order_exact_through_a_program(oracle, programs):
    n, view = 128, (48, 27)
    rng = np.random.default_rng(77)
    prev = np.zeros((n, n, 4), np.float32)
    prev[..., :2] = rng.uniform(-0.3, 0.3, (n, n, 2)) * [1.0, 27 / 48]
    prev[..., 2:] = rng.uniform(-.012, .012, (n, n, 2))
    cur = prev.copy()
    cur[..., :2] += rng.uniform(-.08, .08, (n, n, 2)).astype(np.float32)
    cur[..., 2:] = rng.uniform(-.012, .012, (n, n, 2))
    cur[rng.random((n, n)) < 0.2] = INERT
    base = np.zeros((27, 48, 4), np.float32)
    t = make(n, view, renderView=False, flowShader=programs["flow"])
    t.particles.upload_texels(cur, 0)
    t.particles.upload_texels(prev, 1)
    t.timer.time = 2500.0
    outs = []
    for _ in range(2):                              # (the second run: over the vertex buffer and the scratch the first one left)
        t.flow.set_pixels(base)
        t.draw()
        outs.append((t.flow.read(), t.fragments))
    t.dispose()
    want, frags, cov = oracle.flow_deposit(cur, prev, base, 2500.0, view_size=(1.0, 48 / 27), coverage=True)
    assert cov.max() > 100 and outs[0][1] == outs[1][1] == frags
    assert bits_equal(outs[0][0], want).all() and bits_equal(outs[1][0], want).all()


# ---- 5. nothing of a program pass is reused, nothing is reused by it ------------------------------------------------------------
def stream_context(cur, prev, **options):
    t = make(cur.shape[0], (96, 54), **options)
    t.particles.draw_pipeline("stream")
    t.state.update(speedAlpha=0.5, baseColor=[1, 0.6, 0.2, 0.5])
    t.particles.upload_texels(cur, 0)
    t.particles.upload_texels(prev, 1)
    t.timer.time = 900.0
    t.line_widths()
    return t


def builtin_view(t):
    u, n = t.render_uniforms(), C.c_uint64(0)
    from tendrils_amd import _capi
    _capi.call("th_view_draw", t.particles._ctx, C.byref(u), C.byref(n))
    return int(n.value)


def program_uniforms(t):
    return dict(t.state, time=float(t.timer.time), viewSize=t.viewSize)


def test_no_geometry_is_reused_across_a_program_pass(programs):
    from tendrils_amd import _capi
    cur, prev = random_lines(64, 41, spread=1.0, aspect=54 / 96, inert=0.05)
    # the mirror program into the flow, then the library's view pass with the same viewSize
    t = stream_context(cur, prev)
    mirrored = t._draw_program(programs["mirror"], _capi.TH_PASS_FLOW, program_uniforms(t))
    n = builtin_view(t)
    got = t.read_view()
    t.dispose()
    t = stream_context(cur, prev)                  # ... against a context that never ran a program
    want_n = builtin_view(t)
    want = t.read_view()
    t.dispose()
    assert n == want_n and mirrored > 0 and want.any()
    assert (got == want).all()
    # the converse: the library's flow pass, then the mirror program into the view
    t = stream_context(cur, prev)
    t.particles.deposit_flow(t.viewSize, t.timer.time, t.state["speedLimit"])
    n = t._draw_program(programs["mirror"], _capi.TH_PASS_VIEW, program_uniforms(t))
    got = t.read_view()
    t.dispose()
    t = stream_context(cur, prev)
    want_n = t._draw_program(programs["mirror"], _capi.TH_PASS_VIEW, program_uniforms(t))
    want = t.read_view()
    t.dispose()
    assert n == want_n == mirrored and want.any()
    assert (got == want).all()


# ---- 6. the ring is untouched: a frame loop over sorted slots -------------------------------------------------------------------
def test_frame_loop_with_both_stages_as_programs_equals_the_library(programs):
    n, view = 64, (96, 54)
    rng = np.random.default_rng(5)
    st = np.zeros((n, n, 4), np.float32)
    st[..., :2] = rng.uniform(-0.9, 0.9, (n, n, 2)) * [1.0, 0.5]
    st[..., 2:] = rng.uniform(-.008, .008, (n, n, 2))
    runs = []
    for options in (dict(flowShader=programs["flow"], renderShader=programs["view"]), dict()):
        t = make(n, view, **options)
        assert t.particles.option("bucket", 1) == 1
        t.state["speedAlpha"] = 0.0005
        t.particles.upload_texels(st)
        t.timer.time = 1000.0
        frames = []
        for _ in range(5):
            t.timer.tick()
            t.step()
            t.uniforms["render"]["sinTerm"] = t.render_uniforms().sinTerm
            t.draw()
            frames.append((t.particles.read(0), t.particles.read(1), t.flow.read(), t.read_view(), t.fragments, t.view_fragments))
        t.dispose()
        runs.append(frames)
    for got, want in zip(*runs):
        assert bits_equal(got[0], want[0]).all() and bits_equal(got[1], want[1]).all()
        assert bits_equal(got[2], want[2]).all()
        assert (got[3] == want[3]).all()
        assert got[4] == want[4] and got[5] == want[5]
    assert (runs[1][-1][2][..., 3] != 0).sum() > 500 and runs[1][-1][3].any()


# ---- 7., 8. a packed ring; a width other than 1 ---------------------------------------------------------------------------------
def both_on_one_context(t, cur, prev, base, program):
    """the library's flow pass and the program's on the same context, the flow put back in between: ((flow, n), (flow, n))"""
    from tendrils_amd import _capi
    t.particles.upload_texels(cur, 0)
    t.particles.upload_texels(prev, 1)
    t.timer.time = 321.0
    t.line_widths()
    outs = []
    for run in (lambda: t.particles.deposit_flow(t.viewSize, t.timer.time, t.state["speedLimit"]),
                lambda: t._draw_program(program, _capi.TH_PASS_FLOW, program_uniforms(t))):
        t.flow.set_pixels(base)
        n = run()
        outs.append((t.flow.read(), n))
    return outs


def test_packed_ring_is_seen_as_what_it_decodes_to(programs):
    from tendrils_amd import _capi
    cur, prev = random_lines(100, 16)
    base = np.zeros((54, 96, 4), np.float32)
    t = make(100, (96, 54), stateFormat=_capi.TH_STATE_F16)
    (want, n), (got, frags) = both_on_one_context(t, cur, prev, base, programs["flow"])
    assert not bits_equal(t.particles.read(0), cur).all()
    t.dispose()
    assert frags == n and n > 3000
    assert bits_equal(got, want).all()


def test_the_pass_draws_with_its_line_width(programs):
    cur, prev = random_lines(64, 17, spread=1.0, aspect=54 / 96)
    base = np.zeros((54, 96, 4), np.float32)
    t = make(64, (96, 54), lineWidthRange=(1, 4))
    t.state["flowWidth"] = 3
    (want, n), (got, frags) = both_on_one_context(t, cur, prev, base, programs["flow"])
    t.state["flowWidth"] = 1
    (thin, thin_n), _ = both_on_one_context(t, cur, prev, base, programs["flow"])
    t.dispose()
    assert frags == n and n > 2 * thin_n > 0
    assert bits_equal(got, want).all()


# ---- 9. the accessors -----------------------------------------------------------------------------------------------------------
def tap(u, n):
    return np.clip(np.floor(u * np.float32(n)), 0, n - 1).astype(np.int64)


def stream_states(cur, prev):
    """[2H, W, 4]: the state texel vertex j of column i reads (tendrils_amd/csrc/th_stream.inc, in numpy's fp32)"""
    H, W = cur.shape[:2]
    uvx = (np.arange(W) * (1.0 / (max(W, 2) - 1))).astype(np.float32)
    uvy = (np.arange(2 * H) * (1.0 / (max(2 * H, 2) - 1))).astype(np.float32)
    near = uvy * np.float32(H)
    fl = np.floor(near)
    from_cur = (near - fl) > np.float32(0.25)
    row, col = tap(fl / np.float32(H), H), tap(uvx, W)
    return np.where(from_cur[:, None, None], cur[row][:, col], prev[row][:, col])


def test_th_flow_reads_the_field_as_it_was_before_the_pass(programs):
    n, view = 64, (96, 54)
    cur, prev = random_lines(n, 51, spread=1.0, aspect=54 / 96)
    rng = np.random.default_rng(52)
    base = rng.uniform(-1, 1, (54, 96, 4)).astype(np.float32)
    base[..., 3] = rng.uniform(0, 1, (54, 96))
    got, frags = flow_pass(cur, prev, base, 10.0, view, program=programs["tap"])
    # the same colours looked up here, handed to the same positions as a colour map of the stream's shape
    st = stream_states(cur, prev)
    px, py = st[..., 0] * np.float32(1.0), st[..., 1] * np.float32(96 / 54)
    u, w = px * np.float32(0.5) + np.float32(0.5), py * np.float32(0.5) + np.float32(0.5)
    colours = base[tap(w, 54), tap(u, 96)]
    want, n_want = flow_pass(cur, prev, base, 10.0, view, program=programs["from_map"], prepare=lambda t: t.colorMap.set_pixels(colours))
    assert frags == n_want and frags > 1000
    assert bits_equal(got, want).all() and not bits_equal(got, base).all()


def test_shapes_and_the_colour_map_nobody_uploaded(programs):
    n, view = 64, (96, 54)
    cur, prev = random_lines(n, 53, spread=1.0, aspect=54 / 96)
    base = np.zeros((54, 96, 4), np.float32)
    got, frags = flow_pass(cur, prev, base, 10.0, view, program=programs["shapes"])
    covered = got[..., 3] != 0
    assert frags > 1000 and covered.sum() > 500
    assert (got[covered] == np.float32([96 * 1024 + 54, 1 * 1024 + 1, 0, 1])).all()          # no map: 1 x 1, zeros
    cmap = np.random.default_rng(54).uniform(0, 1, (11, 13, 4)).astype(np.float32)
    got, _ = flow_pass(cur, prev, base, 10.0, view, program=programs["shapes"], prepare=lambda t: t.colorMap.set_pixels(cmap))
    m = cmap[tap(np.float32(0.7), 11), tap(np.float32(0.3), 13)]
    assert (got[covered] == np.float32([96 * 1024 + 54, 13 * 1024 + 11, ((m[0] + m[1]) + m[2]) + m[3], 1])).all()


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------
def test_the_run_entry_points_refuse_each_others_programs(programs):
    from tendrils_amd import _capi
    lib = _capi.load()
    cur, prev = random_lines(32, 61)
    t = make(32, (96, 54))
    t.particles.upload_texels(cur, 0)
    t.particles.upload_texels(prev, 1)
    base = np.random.default_rng(62).uniform(0, 1, (54, 96, 4)).astype(np.float32)
    t.flow.set_pixels(base)
    ctx, n = t.particles._ctx, C.c_uint64(7)
    for other, named in (("state", "state program"), ("screen", "screen program")):
        for which in (_capi.TH_PASS_FLOW, _capi.TH_PASS_VIEW):
            assert lib.th_draw_program_run(ctx, programs[other].handle, None, 0, which, C.byref(n)) == _capi.TH_ERR_INVALID
            said = lib.th_last_error().decode()
            assert "draw program" in said and named in said, said
    assert lib.th_program_run(ctx, programs["flow"].handle, None, 0, _capi.TH_SOURCE_NONE, _capi.TH_TARGET_RING) == _capi.TH_ERR_INVALID
    said = lib.th_last_error().decode()
    assert "draw program" in said and "state program" in said, said
    units = (_capi.ScreenUnit * 1)()
    assert lib.th_screen_run(ctx, programs["flow"].handle, None, 0, units, 0, _capi.SCREEN_TARGET_VIEW, 0, 0) == _capi.TH_ERR_INVALID
    said = lib.th_last_error().decode()
    assert "draw program" in said and "screen program" in said, said
    assert lib.th_draw_program_run(ctx, programs["flow"].handle, None, 0, 2, C.byref(n)) == _capi.TH_ERR_INVALID      # no such pass
    assert bits_equal(t.flow.read(), base).all() and bits_equal(t.particles.read(0), cur).all() and not t.read_view().any()
    # the uniform block: 1024 bytes are taken, 1025 are not
    block = programs["padded"].pack(program_uniforms(t))
    assert C.sizeof(block) == 1024
    assert lib.th_draw_program_run(ctx, programs["padded"].handle, C.byref(block), 1024, _capi.TH_PASS_FLOW, C.byref(n)) == _capi.TH_OK
    assert n.value > 0 and not bits_equal(t.flow.read(), base).all()
    t.flow.set_pixels(base)
    large = (C.c_uint8 * 1025)()
    assert lib.th_draw_program_run(ctx, programs["padded"].handle, large, 1025, _capi.TH_PASS_FLOW, C.byref(n)) == _capi.TH_ERR_INVALID
    assert "1025" in lib.th_last_error().decode()
    assert bits_equal(t.flow.read(), base).all()
    t.dispose()


def test_a_row_band_is_unsupported_and_nothing_is_launched(programs):
    from tendrils_amd import _capi
    lib = _capi.load()
    t = make(64, (96, 54), row0=16, rows=32, globalHeight=64)
    base = np.random.default_rng(63).uniform(0, 1, (54, 96, 4)).astype(np.float32)
    t.flow.set_pixels(base)
    block, n = programs["flow"].pack(program_uniforms(t)), C.c_uint64(7)
    for which in (_capi.TH_PASS_FLOW, _capi.TH_PASS_VIEW):
        status = lib.th_draw_program_run(t.particles._ctx, programs["flow"].handle, C.byref(block), C.sizeof(block), which, C.byref(n))
        assert status == _capi.TH_ERR_UNSUPPORTED, lib.th_last_error()
        assert b"row-band" in lib.th_last_error()
    assert n.value == 7 and bits_equal(t.flow.read(), base).all()
    t.dispose()


# ---- 11. what the compiled stages cost ------------------------------------------------------------------------------------------
def test_query_reports_registers_and_no_scratch(programs):
    from tendrils_amd import _capi
    t = make(32, (96, 54))
    q = _capi.DrawInfo()
    for name in ("flow", "view"):
        info = programs[name].query(t.particles)
        assert info["vgprs"] > 0 and info["sgprs"] > 0 and info["code_bytes"] > 0, info
        assert info["scratch_bytes"] == 0 and info["lds_bytes"] == 0, info
    t._draw_program(programs["flow"], _capi.TH_PASS_FLOW, program_uniforms(t))
    _capi.call("th_draw_query", t.particles._ctx, C.byref(q))
    assert q.pipeline == 0 and q.fragments == 0                # TH_DRAW_STREAM; a fresh ring is inert: nothing drawn
    t.dispose()
