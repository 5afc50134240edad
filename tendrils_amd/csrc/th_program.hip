// th_program.hip - user programs: a caller's HIP pass over the state ring.  The reference is built around this seam -
// Particles.step(update, buffer) runs whatever shader object sits in particles.logic as one full-screen pass
// (src/particles.js:123-145), Tendrils.spawnShader(shader, update, buffer) swaps any gl-shader in for one pass
// (src/index.js:432-457), new Tendrils(gl, { logicShader }) takes a caller's integrator.  Here the caller's shader is HIP
// source for one device function, th_main (th_program_prelude.inc), compiled for gfx950 at run time through hiprtc and run
// with the ring semantics of th_step and the spawn passes (th_spawn.hip: spawn_from_data).
//
// hiprtc is bound at run time like librccl in th_comm.hip: the copy the process already holds (torch's, in the Python host),
// else by soname; TH_HIPRTC_LIB names another.  Nothing here is linked against it: a host that never compiles a program never
// loads it, and compiling needs no device.
//
// What the kinds of program share (th_screen.hip: screen programs; th_drawprog.hip: draw programs; th_stepprog.hip: step programs; th_fragprog.hip: fragment programs; th_measure.hip: measure programs) is here too: the hiprtc binding, the compile, the log,
// what is read out of the code object, the per-context modules (thi::program_*).  What a kind is called and which kernels its
// module holds stands in one table (th_program_kinds.hpp).
#include <dlfcn.h>
#include <elf.h>
#include <hip/hiprtc.h>

#include "th_ctx.hpp"

using namespace thi;

namespace {

const char kPrelude[] =
#include "th_program_prelude.inc"
    ;

// the launch record (th_program_prelude.inc: th_program_args, th_program_uniform_block - the same layout)
struct ProgramArgs {
    const float4 *particles;
    float4 *out;
    const float4 *data, *flow, *targets;
    unsigned *flag;
    uint32_t count, width, rows, row0, global_height;
    int32_t dw, dh, fw, fh;
    uint32_t reserved[3];
};
using KernArgs = ProgramKernArgs<ProgramArgs>;
static_assert(sizeof(ProgramArgs) == 96 && offsetof(KernArgs, u) == 96 && sizeof(KernArgs) == 96 + kUniformBytes,
              "launch record: layout shared with th_program_prelude.inc");

struct Hiprtc {
    void *lib = nullptr;
    std::string where, error;
    decltype(&hiprtcCreateProgram) CreateProgram = nullptr;
    decltype(&hiprtcCompileProgram) CompileProgram = nullptr;
    decltype(&hiprtcDestroyProgram) DestroyProgram = nullptr;
    decltype(&hiprtcGetProgramLogSize) GetProgramLogSize = nullptr;
    decltype(&hiprtcGetProgramLog) GetProgramLog = nullptr;
    decltype(&hiprtcGetCodeSize) GetCodeSize = nullptr;
    decltype(&hiprtcGetCode) GetCode = nullptr;
    decltype(&hiprtcGetErrorString) GetErrorString = nullptr;
};

Hiprtc &hiprtc()
{
    static Hiprtc r;
    static std::once_flag once;
    std::call_once(once, [] {
        const char *env = getenv("TH_HIPRTC_LIB");
        const char *names[] = {env, "libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"};
        // RTLD_NOLOAD over every name first: a copy the process already holds wins over a second one from another path
        for (int pass = 0; pass < 2 && !r.lib; ++pass)
            for (const char *n : names) {
                if (!n || !*n) continue;
                void *h = dlopen(n, pass == 0 && n != env ? RTLD_NOW | RTLD_NOLOAD : RTLD_NOW | RTLD_LOCAL);
                if (h) { r.lib = h; r.where = n; break; }
                if (pass == 0) continue;
                const char *e = dlerror();
                r.error += std::string(r.error.empty() ? "" : "; ") + n + ": " + (e ? e : "?");
            }
        if (!r.lib) return;
        bool all = true;
#define TH_SYM(f) do { r.f = reinterpret_cast<decltype(r.f)>(dlsym(r.lib, "hiprtc" #f)); if (!r.f) { all = false; r.error += " missing hiprtc" #f; } } while (0)
        TH_SYM(CreateProgram); TH_SYM(CompileProgram); TH_SYM(DestroyProgram); TH_SYM(GetProgramLogSize); TH_SYM(GetProgramLog);
        TH_SYM(GetCodeSize); TH_SYM(GetCode); TH_SYM(GetErrorString);
#undef TH_SYM
        if (!all) { dlclose(r.lib); r.lib = nullptr; }
    });
    return r;
}

thread_local std::string g_program_log;

// What the code object says of the kind's kernel: the SGPR count is in its metadata note alone (msgpack: the kernel's map has
// its keys in order, .name before .sgpr_count), the code size is that of .text.
void inspect_code_object(th_program *p)
{
    const std::vector<char> &b = p->code;
    if (b.size() >= sizeof(Elf64_Ehdr) && !memcmp(b.data(), ELFMAG, SELFMAG)) {
        Elf64_Ehdr eh;
        memcpy(&eh, b.data(), sizeof eh);
        if (eh.e_shentsize == sizeof(Elf64_Shdr) && eh.e_shstrndx < eh.e_shnum &&
            eh.e_shoff <= b.size() && (size_t)eh.e_shnum * sizeof(Elf64_Shdr) <= b.size() - eh.e_shoff) {
            std::vector<Elf64_Shdr> sh(eh.e_shnum);
            memcpy(sh.data(), b.data() + eh.e_shoff, sh.size() * sizeof(Elf64_Shdr));
            const Elf64_Shdr &names = sh[eh.e_shstrndx];
            for (const Elf64_Shdr &s : sh) {
                if (names.sh_offset > b.size() || s.sh_name >= names.sh_size || names.sh_size > b.size() - names.sh_offset) continue;
                const char *n = b.data() + names.sh_offset + s.sh_name;
                if (!strncmp(n, ".text", names.sh_size - s.sh_name) && s.sh_type == SHT_PROGBITS) p->code_bytes = (uint32_t)s.sh_size;
            }
        }
    }
    const char *const kernel = kProgramKindTable[p->kind].entry[0];
    const std::string name = std::string(1, (char)(0xa0 + strlen(kernel))) + kernel, key = "\xab.sgpr_count";
    auto at = std::search(b.begin(), b.end(), name.begin(), name.end());
    if (at != b.end()) at = std::search(at, b.end(), key.begin(), key.end());
    if (at == b.end() || (size_t)(b.end() - at) < key.size() + 5) return;
    const unsigned char *v = reinterpret_cast<const unsigned char *>(&*at) + key.size();
    if (v[0] < 0x80) p->sgprs = v[0];
    else if (v[0] == 0xcc) p->sgprs = v[1];
    else if (v[0] == 0xcd) p->sgprs = (uint32_t)v[1] << 8 | v[2];
    else if (v[0] == 0xce) p->sgprs = (uint32_t)v[1] << 24 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 8 | v[4];
}

}  // namespace

namespace thi {

void program_release(th_program *p)
{
    if (p && p->refs.fetch_sub(1) == 1) delete p;
}

void ProgramModule::reset()
{
    if (module) (void)hipModuleUnload(module);
    program_release(prog);
    module = nullptr; prog = nullptr;
    for (hipFunction_t &fn : entry) fn = nullptr;
}

th_status program_run_args(const th_program *prog, ProgramKind kind, const char *entry, const void *uniforms, uint32_t uniform_bytes)
{
    TH_REQUIRE(prog, "null program");
    TH_REQUIRE(prog->kind == kind, "%s runs a %s: '%s' is a %s", entry, program_kind_name(kind), prog->name.c_str(), program_kind_name(prog->kind));
    TH_REQUIRE(uniform_bytes <= kUniformBytes, "uniform block of %u bytes (at most %u)", uniform_bytes, kUniformBytes);
    TH_REQUIRE(uniforms || uniform_bytes == 0, "null uniforms");
    return TH_OK;
}

th_status program_loaded(th_context *c, th_program *prog, ProgramModule **out)
{
    for (const std::unique_ptr<ProgramModule> &m : c->programs) if (m->prog == prog) { *out = m.get(); return TH_OK; }
    std::lock_guard<std::mutex> hold(prog->lock);
    TH_REQUIRE(!prog->destroyed, "program '%s' was destroyed before this context had loaded it", prog->name.c_str());
    std::unique_ptr<ProgramModule> m(new ProgramModule);
    TH_HIP(hipModuleLoadData(&m->module, prog->code.data()));
    const ProgramKindInfo &kind = kProgramKindTable[prog->kind];
    for (int e = 0; e < kind.entries; ++e) TH_HIP(hipModuleGetFunction(&m->entry[e], m->module, kind.entry[e]));
    m->prog = prog;
    prog->refs.fetch_add(1);
    c->programs.push_back(std::move(m));
    *out = c->programs.back().get();
    return TH_OK;
}

th_status program_launch(th_context *c, hipFunction_t fn, size_t lanes, void *record, size_t bytes)
{
    return program_launch_grid(c, fn, th::grid_for(lanes, 8), record, bytes);
}

th_status program_launch_grid(th_context *c, hipFunction_t fn, int grid, void *record, size_t bytes, int grid_y)
{
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, record, HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes, HIP_LAUNCH_PARAM_END};
    TH_HIP(hipModuleLaunchKernel(fn, (unsigned)grid, (unsigned)grid_y, 1, 256, 1, 1, 0, c->stream, nullptr, extra));
    return TH_OK;
}

th_status program_compile(ProgramKind kind, const std::string &prelude, const char *source, const char *name, th_program **out)
{
    TH_REQUIRE(source && out, "null argument");
    *out = nullptr;
    g_program_log.clear();
    Hiprtc &R = hiprtc();
    if (!R.lib) return fail(TH_ERR_UNSUPPORTED, "hiprtc is not loadable (%s); TH_HIPRTC_LIB names one", R.error.c_str());
    const std::string label = name && *name ? name : "user_program";
    // the user's text begins at line 1 of a file called `label`: a diagnostic names the line the user wrote
    const std::string text = prelude + "\n#line 1 \"" + label + "\"\n" + source + "\n";
    hiprtcProgram hp = nullptr;
    hiprtcResult r = R.CreateProgram(&hp, text.c_str(), kProgramKindTable[kind].prelude, 0, nullptr, nullptr);
    if (r != HIPRTC_SUCCESS) return fail(TH_ERR_INVALID, "hiprtcCreateProgram: %s", R.GetErrorString(r));
    // the product's arithmetic flags (csrc/Makefile: HIPFLAGS)
    const char *opts[] = {"-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "--offload-arch=gfx950"};
    r = R.CompileProgram(hp, (int)(sizeof opts / sizeof *opts), opts);
    size_t n = 0;
    if (R.GetProgramLogSize(hp, &n) == HIPRTC_SUCCESS && n > 1) {
        g_program_log.resize(n);
        if (R.GetProgramLog(hp, &g_program_log[0]) != HIPRTC_SUCCESS) g_program_log.clear();
        while (!g_program_log.empty() && g_program_log.back() == '\0') g_program_log.pop_back();
    }
    th_program *p = nullptr;
    th_status st = TH_OK;
    if (r != HIPRTC_SUCCESS) {
        st = fail(TH_ERR_INVALID, "program '%s' does not compile (%s): th_program_log() has the compiler's output", label.c_str(), R.GetErrorString(r));
    } else if ((r = R.GetCodeSize(hp, &n)) != HIPRTC_SUCCESS || n == 0) {
        st = fail(TH_ERR_INVALID, "hiprtcGetCodeSize: %s", R.GetErrorString(r));
    } else if (!(p = new (std::nothrow) th_program)) {
        st = fail(TH_ERR_INVALID, "out of host memory");
    } else {
        p->kind = kind;
        p->name = label;
        p->code.resize(n);
        if ((r = R.GetCode(hp, p->code.data())) != HIPRTC_SUCCESS) {
            st = fail(TH_ERR_INVALID, "hiprtcGetCode: %s", R.GetErrorString(r));
            delete p;
            p = nullptr;
        } else inspect_code_object(p);
    }
    (void)R.DestroyProgram(&hp);
    *out = p;
    return st;
}

}  // namespace thi

extern "C" {

const char *th_program_log(void) { return g_program_log.c_str(); }

th_status th_program_compile(const char *source, const char *name, th_program **out)
{
    return program_compile(kStateProgram, kPrelude, source, name, out);
}

th_status th_program_destroy(th_program *p)
{
    if (!p) return TH_OK;
    {
        std::lock_guard<std::mutex> hold(p->lock);
        TH_REQUIRE(!p->destroyed, "program destroyed twice");
        p->destroyed = true;
        std::vector<char>().swap(p->code);        // (the contexts that loaded it hold modules of their own)
    }
    program_release(p);
    return TH_OK;
}

th_status th_program_run(th_context *c, th_program *prog, const void *uniforms, uint32_t uniform_bytes, int32_t source, int32_t target)
{
    if (th_status s = use(c)) return s;
    if (th_status s = program_run_args(prog, kStateProgram, "th_program_run", uniforms, uniform_bytes)) return s;
    ProgramModule *m = nullptr;
    if (th_status s = program_loaded(c, prog, &m)) return s;
    if (th_status s = ensure_identity(c)) return s;      // a pass operates in texel order, like every spawn pass
    TH_REQUIRE(c->ring.size() >= 2, "a pass needs at least 2 state buffers (have %zu)", c->ring.size());
    const bool band = c->cfg.height != c->cfg.global_height;
    if (!c->prog_flag) {
        if (th_status s = c->prog_flag.alloc(1)) return s;
        TH_HIP(hipMemsetAsync(c->prog_flag, 0, sizeof(unsigned), c->stream));
    }
    RingPass pass;
    if (th_status s = pass.begin(c, target)) return s;
    KernArgs k{};
    k.a.particles = pass.particles;
    k.a.out = pass.rt;
    if (th_status s = spawn_data(c, source, pass.particles, true, &k.a.data, &k.a.dw, &k.a.dh)) return s;
    k.a.flow = c->flow; k.a.fw = c->fw; k.a.fh = c->fh;
    k.a.targets = c->targets;
    k.a.flag = c->prog_flag;
    k.a.count = (uint32_t)c->texels(); k.a.width = (uint32_t)c->cfg.width; k.a.rows = (uint32_t)c->cfg.height;
    k.a.row0 = (uint32_t)c->cfg.row0; k.a.global_height = (uint32_t)c->cfg.global_height;
    k.set_uniforms(uniforms, uniform_bytes);
    if (th_status s = program_launch(c, m->entry[kStateRun], c->texels(), k)) return s;
    if (th_status s = pass.commit(c)) return s;
    if (band) {
        // only a row band can be asked for rows it does not hold: checked like the sharded spawn's out-of-band flag
        unsigned flag = 0;
        if (th_status s = read_back(c, &flag, c->prog_flag, sizeof flag)) return s;
        if (flag) {
            TH_HIP(hipMemsetAsync(c->prog_flag, 0, sizeof(unsigned), c->stream));
            return fail(TH_ERR_UNSUPPORTED, "program '%s' read row %u of `particles` on a row band that holds rows %d..%d (up to row %u): a pass cannot fetch other bands' texels",
                        m->prog->name.c_str(), flag - 1, c->cfg.row0, c->cfg.row0 + c->cfg.height - 1, flag - 1);
        }
    }
    return TH_OK;
}

th_status th_program_query(th_context *c, th_program *prog, th_program_info *info)
{
    if (th_status s = use(c, true)) return s;
    TH_REQUIRE(prog && info, "null argument");
    ProgramModule *m = nullptr;
    if (th_status s = program_loaded(c, prog, &m)) return s;
    int vgprs = 0, lds = 0, scratch = 0;
    const hipFunction_t first = m->entry[0];          // (the kind's first kernel, whose SGPRs and code size the compile read)
    TH_HIP(hipFuncGetAttribute(&vgprs, HIP_FUNC_ATTRIBUTE_NUM_REGS, first));
    TH_HIP(hipFuncGetAttribute(&lds, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, first));
    TH_HIP(hipFuncGetAttribute(&scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, first));
    info->vgprs = (uint32_t)vgprs; info->sgprs = m->prog->sgprs;
    info->lds_bytes = (uint32_t)lds; info->scratch_bytes = (uint32_t)scratch; info->code_bytes = m->prog->code_bytes;
    return TH_OK;
}

}  // extern "C"
