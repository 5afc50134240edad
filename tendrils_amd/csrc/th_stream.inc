// th_stream.inc - the vertex stream of Particles.draw: which state texel, of which buffer, vertex j of column i of the stream
// Particles.generateLUT([W, 2H]) reads through src/state/state-at-frame.glsl:12-22.  ONE copy, read twice, as th_taps.inc
// (whose th_tap_nearest it uses: that file comes first).  The includer defines TH_STREAM:
//   th_raster.hpp    #define TH_STREAM(...) __VA_ARGS__     the function itself (namespace th): dep_fetch looks its texel up with it
//   th_drawprog.hip  #define TH_STREAM(...) #__VA_ARGS__    its text, handed to hiprtc in front of the draw prelude
// Hence: no preprocessor directive and no project name inside TH_STREAM( ), only what hipcc and hiprtc both know.
TH_STREAM(
template <class T> struct th_stream_at {
    float uvx, uvy;          // the attribute: a Float32Array of JS doubles
    int row, col;            // the texel the lookup lands on: not always the line's own - heights such as 100, and 8192 and more,
                             // drift.  row: counted from row0, the first row the buffers hold (a row band; else 0)
    bool from_cur;           // ... of `current` (else of `previous`)
    const T *tex;            // ... that buffer
};
template <class T>
__device__ __forceinline__ th_stream_at<T> th_stream_lookup(unsigned i, unsigned j, double inv_x, double inv_y, int W, int H, unsigned row0,
                                                            const T *cur, const T *prev)
{
    th_stream_at<T> s;
    s.uvx = (float)((double)i * inv_x);
    s.uvy = (float)((double)j * inv_y);
    const float near_index = s.uvy * (float)H;
    const float fl = __builtin_floorf(near_index);
    const float offset = near_index - fl;
    const float ly = fl / (float)H;
    s.tex = offset > 0.25f ? cur : prev;
    s.from_cur = offset > 0.25f;
    s.row = th_tap_nearest(ly, H) - (int)row0;
    s.col = th_tap_nearest(s.uvx, W);
    return s;
}
)
