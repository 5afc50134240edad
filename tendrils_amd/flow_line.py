"""Flow lines: strokes drawn into tendrils.flow - the reference's FlowLine / FlowLines (src/flow-line/index.js, multi.js).

A FlowLine is a path of points (NDC, f32) with a time (ms) per point.  update() builds the triangle strip's attributes
(th_flow_line_attributes: Line.update() + FlowLine.setAttributes); draw() draws the strip as it was at the last update()
into the flow texture bound last (`tendrils.flow.bind()`, as the demo does before drawing its lines) or into an explicit
target, through th_flow_lines.  FlowLines keeps one line per id; its `active` iterates in a JS object's key order (integer
ids ascending, then other ids in insertion order), which is the order the demo draws them in.

    tendrils.step(); tendrils.draw()
    tendrils.flow.bind()
    lines.trim(1 / tendrils.state["flowDecay"], tendrils.timer.time)
    for fl in lines.active.values():
        fl.line.uniforms.update(tendrils.state); fl.update().draw()
"""
import ctypes as C
import time as _time
from collections.abc import MutableMapping

import numpy as np

from . import _capi
from ._capi import call

# Line's defaults (src/geom/line/index.js:15-29) with FlowLine's (src/flow-line/index.js:18-21) over them
def defaults():
    return {"color": [1.0, 1.0, 1.0, 1.0], "rad": 0.1, "viewSize": [1.0, 1.0],
            "speed": 3.0, "speedLimit": 0.01, "crestShape": 0.6}


ATTRIBUTES = ("position", "normal", "miter", "previous", "time", "dt")
_bound = [None]          # the flow texture FlowTexture.bind() bound last (GL: the bound framebuffer)


def bind(flow):
    """Make `flow` (a tendrils_amd.tendrils.FlowTexture) the target of draw() calls without an explicit one."""
    _bound[0] = flow
    return flow


def _target(target):
    t = target if target is not None else _bound[0]
    if t is None:
        raise RuntimeError("no flow texture bound: call tendrils.flow.bind() or pass draw(target)")
    owner = getattr(t, "_o", None)
    if owner is None or owner.particles is None:
        raise RuntimeError("the flow texture's Tendrils has no particles (call setup() first)")
    return owner.particles._ctx


def uniforms_struct(u):
    s = _capi.FlowLineUniforms()
    s.speed, s.rad, s.crestShape, s.speedLimit = float(u["speed"]), float(u["rad"]), float(u["crestShape"]), float(u["speedLimit"])
    s.viewSize[0], s.viewSize[1] = float(u["viewSize"][0]), float(u["viewSize"][1])
    return s


def attributes(points, times, closed=False):
    """The strip's attribute arrays (dict of f32 arrays: position/normal/previous [V,2], miter/time/dt [V]) of one line."""
    pts = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 2))
    tms = np.ascontiguousarray(np.asarray(times, np.float64).reshape(-1))
    if len(tms) != len(pts):
        raise ValueError("%d points but %d times" % (len(pts), len(tms)))
    nv = C.c_int32(0)
    _dp = C.POINTER(C.c_double)
    call("th_flow_line_attributes", pts.ctypes.data_as(_capi._fp), tms.ctypes.data_as(_dp), len(pts), int(bool(closed)),
         0, C.byref(nv), None, None, None, None, None, None)
    out = {k: np.zeros((nv.value, 2) if k in ("position", "normal", "previous") else (nv.value,), np.float32) for k in ATTRIBUTES}
    if nv.value:
        call("th_flow_line_attributes", pts.ctypes.data_as(_capi._fp), tms.ctypes.data_as(_dp), len(pts), int(bool(closed)),
             nv.value, C.byref(nv), *[out[k].ctypes.data_as(_capi._fp) for k in ATTRIBUTES])
    return out


def draw_lines(ctx, uniforms, lines):
    """One th_flow_lines call: `lines` = [(points [n,2] f32, times [n] f64, closed)...] in draw order."""
    if not lines:
        return call("th_flow_lines", ctx, C.byref(uniforms_struct(uniforms)), None, None, None, None, 0)
    pts = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float32).reshape(-1, 2) for p, _, _ in lines]))
    tms = np.ascontiguousarray(np.concatenate([np.asarray(t, np.float64).reshape(-1) for _, t, _ in lines]))
    offs = np.ascontiguousarray(np.cumsum([0] + [len(t) for _, t, _ in lines]), np.int32)
    closed = np.ascontiguousarray([int(bool(c)) for _, _, c in lines], np.int32)
    _ip = C.POINTER(C.c_int32)
    return call("th_flow_lines", ctx, C.byref(uniforms_struct(uniforms)), pts.ctypes.data_as(_capi._fp),
                tms.ctypes.data_as(C.POINTER(C.c_double)), offs.ctypes.data_as(_ip), closed.ctypes.data_as(_ip), len(lines))


class Line:
    """The geometry half of a FlowLine (src/geom/line/index.js): path, closed, uniforms, the drawn attributes."""

    def __init__(self, uniforms=None, path=None, closed=False):
        self.uniforms = uniforms if uniforms is not None else defaults()
        self.path = path if path is not None else []
        self.closed = bool(closed)
        self.attributes = None
        self._drawn = None           # (points, times, closed) as of the last update(): what draw() draws

    def update(self, times):
        pts = np.asarray(self.path, np.float32).reshape(-1, 2)
        tms = np.asarray(times[:len(self.path)], np.float64)
        self.attributes = attributes(pts, tms, self.closed)
        self._drawn = (pts.copy(), tms.copy(), self.closed)
        return self


class FlowLine:
    """src/flow-line/index.js: FlowLine(options) with options uniforms / path / closed / times."""

    def __init__(self, options=None):
        o = dict(options or {})
        self.line = Line(o["uniforms"] if "uniforms" in o else defaults(), o.get("path") or [], o.get("closed", False))
        self.times = o.get("times") or []

    def update(self):
        self.line.update(self.times)
        return self

    def draw(self, target=None):
        """Draws the strip of the last update() (nothing while the path is empty, as Line.draw)."""
        if len(self.line.path) > 0 and self.line._drawn is not None:
            draw_lines(_target(target), self.line.uniforms, [self.line._drawn])
        return self

    def add(self, time, point):
        self.times.append(time)
        self.line.path.append(point)
        return self

    def insert(self, time, point):
        i = self.findIndex(time)
        self.times.insert(i, time)
        self.line.path.insert(i, point)
        return self

    def at(self, index, out=None):
        out = {} if out is None else out
        out["time"] = self.times[index] if -len(self.times) <= index < len(self.times) else None
        out["point"] = self.line.path[index] if -len(self.line.path) <= index < len(self.line.path) else None
        return out

    def findIndex(self, time):
        for i, t in enumerate(self.times):
            if t > time:
                return i
        return len(self.times)

    def trim(self, ago, now=None):
        """Drops the points older than `now - ago` (ms) from the front; returns the remaining length."""
        now = _time.time() * 1000.0 if now is None else now
        oldest = now - ago
        while self.times and self.times[0] < oldest:
            self.times.pop(0)
            self.line.path.pop(0)
        return self.length

    @property
    def length(self):
        return len(self.times)


def _js_key(k):
    """A JS object's property key: ids become strings (3 and "3" are the same key)."""
    if isinstance(k, bool):
        return "true" if k else "false"
    if isinstance(k, float) and k.is_integer():
        k = int(k)
    return str(k)


def _array_index(k):
    return k.isdigit() and str(int(k)) == k and int(k) < 4294967295


class JsObject(MutableMapping):
    """A plain JS object's key order: array-index keys ascending, then the other keys in insertion order."""

    def __init__(self):
        self._d = {}

    def __getitem__(self, k):
        return self._d[_js_key(k)]

    def __setitem__(self, k, v):
        self._d[_js_key(k)] = v

    def __delitem__(self, k):
        del self._d[_js_key(k)]

    def __contains__(self, k):
        return _js_key(k) in self._d

    def __iter__(self):
        keys = list(self._d)
        return iter(sorted((k for k in keys if _array_index(k)), key=int) + [k for k in keys if not _array_index(k)])

    def __len__(self):
        return len(self._d)

    def __repr__(self):
        return "JsObject(%r)" % dict(self.items())


class FlowLines:
    """src/flow-line/multi.js: one FlowLine per id."""

    def __init__(self):
        self.active = JsObject()

    def get(self, id, options=None):
        if id not in self.active or not self.active[id]:
            self.active[id] = FlowLine(options)
        return self.active[id]

    def trim(self, *times):
        """Trims every line (FlowLine.trim(*times)) and deletes the ones left empty; returns how many remain."""
        remaining = 0
        for k in list(self.active):
            if self.active[k].trim(*times) == 0:
                del self.active[k]
            else:
                remaining += 1
        return remaining

    def draw(self, target=None, update=True):
        """update() (optional) and draw() of every active line in order, in as few th_flow_lines calls as their uniforms
        allow (consecutive lines with equal uniforms share one call)."""
        ctx = _target(target)
        run, run_u = [], None
        for fl in self.active.values():
            if update:
                fl.update()
            if not fl.line.path or fl.line._drawn is None:
                continue
            u = uniforms_struct(fl.line.uniforms)
            key = bytes(u)
            if run and key != run_u:
                draw_lines(ctx, run[0][0], [d for _, d in run])
                run = []
            run.append((fl.line.uniforms, fl.line._drawn))
            run_u = key
        if run:
            draw_lines(ctx, run[0][0], [d for _, d in run])
        return self
