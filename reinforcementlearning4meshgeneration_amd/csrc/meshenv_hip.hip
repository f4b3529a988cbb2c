// meshenv_hip.hip -- C-ABI (include/meshenv.h) over the wave-per-environment kernels.
//
// Host side: owns the HBM state of a batch of environments, launches k_init_domains / k_reset / k_step on
// the handle's stream.  Nothing here computes environment results on the host: without a working GPU every
// entry point fails with MESHENV_E_HIP.
#include "../../include/meshenv.h"
#include "../../include/meshenv_optim.h"
#include "../../include/meshenv_td3_actor_grad.h"
#include "../../include/meshenv_ppo_grad.h"
#include "../../include/meshenv_rollout.h"
#include "../../include/meshenv_onpolicy_train.h"
#include "../../include/meshenv_onpolicy_learn.h"
#include "../../include/meshenv_offpolicy_train.h"
#include "../../include/meshenv_offpolicy_learn.h"
#include "../../include/meshenv_eval_callback.h"
#include "../../include/meshenv_topology.h"
#include "../../include/meshenv_fnn.h"
#include "../../include/meshenv_fnn_train.h"
#include "../../include/meshenv_augment.h"
#include "../../include/meshenv_ddpg.h"
#include "../../include/meshenv_ddpg_grad.h"

#include <hip/hip_runtime.h>
#include <link.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "meshenv_actor.h"
#include "meshenv_domgen.h"
#include "meshenv_kernels.h"
#include "meshenv_quality.h"
#include "meshenv_smooth.h"
#include "meshenv_samples.h"
#include "meshenv_fused.h"
#include "meshenv_policy.h"
#include "meshenv_gae.h"
#include "meshenv_eval.h"
#include "meshenv_replay.h"
#include "meshenv_target.h"
#include "meshenv_wide.h"
#include "meshenv_critic_grad.h"
#include "meshenv_actor_grad.h"
#include "meshenv_td3_actor_grad.h"
#include "meshenv_wide_grad.h"
#include "meshenv_ppo_grad.h"
#include "meshenv_optim.h"
#include "meshenv_rollout.h"
#include "meshenv_onpolicy_train.h"
#include "meshenv_offpolicy_train.h"
#include "meshenv_learn.h"
#include "meshenv_eval_callback.h"
#include "meshenv_topology.h"
#include "meshenv_fnn.h"
#include "meshenv_fnn_grad.h"
#include "meshenv_augment.h"
#include "meshenv_step_variant.h"
#include "meshenv_grad_bind.h"

using namespace meshenv;

namespace {
thread_local std::string g_create_error;

// ---- glibc's atan2, restated (csrc/meshenv_libm.h): the 241 x 7 table comes out of the libm image of this process.
// A record is {x_i, atan(x_i), 1 / (1 + x_i^2), ...} with x_i within 1/256 of (i + 16) / 256; the scan accepts the first
// 8-byte-aligned run of 241 such records in a readable segment of libm.so.
struct AtanHost {
    std::vector<double> cij;   // empty: not found
    int mode = 0;              // 2 restated glibc validated against this libm, 1 correctly rounded (atan2_cr), 0 ocml only
};

static bool atan_row_ok(const double *r, int i)
{
    const double x = r[0];
    if (!(std::fabs(x - (i + 16) / 256.0) < 1.0 / 256.0)) return false;
    return std::fabs(r[1] - std::atan(x)) < 1e-15 && std::fabs(r[2] * (1.0 + x * x) - 1.0) < 1e-12;
}

static int atan_scan_cb(struct dl_phdr_info *info, size_t, void *data)
{
    AtanHost *st = (AtanHost *)data;
    if (!st->cij.empty() || !info->dlpi_name || !std::strstr(info->dlpi_name, "libm.so")) return 0;
    const size_t bytes = sizeof(double) * kAtanRows * kAtanCols;
    for (int k = 0; k < info->dlpi_phnum; k++) {
        const ElfW(Phdr) *ph = &info->dlpi_phdr[k];
        if (ph->p_type != PT_LOAD || !(ph->p_flags & PF_R) || ph->p_memsz < bytes) continue;
        const unsigned char *base = (const unsigned char *)(info->dlpi_addr + ph->p_vaddr);
        size_t o = (8 - ((uintptr_t)base & 7)) & 7;
        for (; o + bytes <= ph->p_memsz; o += 8) {
            double r[3];
            std::memcpy(r, base + o, sizeof r);
            if (!(r[0] > 0.06 && r[0] < 0.07) || !atan_row_ok(r, 0)) continue;
            std::vector<double> t((size_t)kAtanRows * kAtanCols);
            std::memcpy(t.data(), base + o, bytes);
            bool all = true;
            for (int i = 0; i < kAtanRows && all; i++) all = atan_row_ok(t.data() + (size_t)kAtanCols * i, i);
            if (all) { st->cij.swap(t); return 1; }
        }
    }
    return 0;
}

// atan2_glibc against the atan2 of this process on 2^18 arguments: all four octants, both the polynomial (u < 1/16) and
// the table branch, lattice (4-decimal) and unrestricted coordinates, and the half-quantum angles the front smoother builds.
static bool atan_validate(const std::vector<double> &cij)
{
    unsigned long long s = 0x9E3779B97F4A7C15ULL;
    auto next = [&s]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    auto unit = [&next]() { return (double)(next() >> 11) / 9007199254740992.0; };
    for (int n = 0; n < (1 << 18); n++) {
        double y = 6.0 * unit() - 3.0, x = 6.0 * unit() - 3.0;
        const int kind = n & 3;
        if (kind == 1) { y = std::round(y * 1e4) / 1e4; x = std::round(x * 1e4) / 1e4; }
        else if (kind == 2) y = std::ldexp(y, (int)(next() % 60) - 30);
        else if (kind == 3) {
            const double h = ((double)(next() % 62832) + 0.5) * 1e-4, sc = 0.01 + 3.0 * unit();
            y = -std::sin(h) * sc; x = std::cos(h) * sc;
        }
        bool ok = false;
        const double mine = atan2_glibc(y, x, cij.data(), ok);
        if (ok && f64_bits(mine) != f64_bits(std::atan2(y, x))) return false;
    }
    return true;
}

static const AtanHost &atan_host()
{
    static AtanHost st;
    static std::once_flag once;
    std::call_once(once, [] {
        const char *off = std::getenv("MESHENV_LIBM_EXACT");   // "0": ocml's atan2 everywhere (as before round 3)
        if (off && off[0] == '0') { st.mode = 0; return; }
        volatile double one = 1.0;
        (void)std::atan2(one, one);   // keeps libm's atan2 linked and resolved
        dl_iterate_phdr(atan_scan_cb, &st);
        st.mode = (!st.cij.empty() && atan_validate(st.cij)) ? 2 : 1;
    });
    return st;
}

// table + mode into the current device's copy of the module globals (13.5 KB; every handle creation and selftest does it)
static hipError_t upload_atan_state()
{
    const AtanHost &st = atan_host();
    hipError_t e = hipSuccess;
    if (st.mode == 2) e = hipMemcpyToSymbol(HIP_SYMBOL(g_atan_cij), st.cij.data(), sizeof(double) * st.cij.size());
    const int mode = st.mode;
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_atan_mode), &mode, sizeof mode);
    return e;
}
}

struct MeshEnv {
    int device = 0;
    hipStream_t stream = nullptr;
    DevState S{};
    int n_envs = 0, n_domains = 0, cap = 0, max_ring = 0;
    uint64_t steps_done = 0;  // vector steps executed so far (index of the next step)
    DevCold cold{};  // host copy of *S.cold
    bool default_params = true;  // geometry constants are the reference's: literal-constant kernel instantiations
    size_t lds = 0;
    int n_cu = 256;       // compute units of the device (hipDeviceAttributeMultiprocessorCount)
    int group = 1;        // environments (wavefronts) per workgroup of the single-step kernel
    size_t group_lds = 0;
    int2 *env_lds = nullptr;   // ragged LDS packing of the CU-group kernel: [n_envs] (byte offset in the workgroup, ring slots), or null
    int ho_off = 0;            // ragged: offset of the hand-over blocks
    std::vector<int2> env_lds_host;
    std::vector<int32_t> dom_off_host, env_dom_host;
    std::vector<void *> allocs;
    std::string err;
    int timing = 0;              // 0 = off, k = bracket every other group of k consecutive launches
    long long launch_count = 0;
    std::vector<hipEvent_t> ev;  // 2 * MESHENV_TIMING_POOL events, created on first use
    int32_t *smooth_sweeps = nullptr;  // [E], allocated by the first meshenv_smooth: what the smoother did per env
    int32_t *front_code = nullptr;     // [E] outcome of the front smoother (gates the interior pass of the same call)
    double *front_tab = nullptr;       // [kFtTotal] the front smoother's tan / cos values from the host's libm
    bool smooth_ready = false, move_ready = false;   // set only after every allocation / attribute call succeeded
    int libm_exact = -1;               // pow2_glibc == the running libm's pow(x, 2.0) on the validation set (-1: not checked yet)
    Reselect *pend = nullptr;          // [E] selection parked by the candidate rebuild (csrc/meshenv_smooth.h)
    float *pend_obs = nullptr;         // [E][18]
    bool reselect_pending = false;     // a rebuild ran since the last step kernel
    bool front_moved = false;          // a front smoother ran since the last full reset: rings may hold off-lattice vertices
    bool smooth_final_ready = false;
    bool fused_ready = false;          // k_step_group_actor's LDS attribute set
    int stage_bits = 0;                // bits 1 | 2 of k_step's auto_reset argument: record-first / key-less staging (set at creation)
    bool samples_ready = false;        // k_extract_samples' LDS attribute set
    // move() API state, allocated by the first meshenv_move: not_valid_points per env
    double2 *nv_xy = nullptr;    // [E][cap]
    int32_t *nv_count = nullptr; // [E]
    int32_t *nv_gid = nullptr;   // [E][cap] ring id of each listed vertex (identity, for last_not_valid_points)
    int32_t *nv_meta = nullptr;  // [E][kNvMeta] episode counter + last_not_valid_points summary
    uint8_t *move_mask = nullptr;  // [E] envs of the last meshenv_move that went through smooth_pave
    long long ev_count = 0;      // launches recorded since timing was armed
    // meshenv_evaluate's step buffers (allocated by its first call without caller buffers) and the pinned host word it
    // reads the short-envs counter into
    float *eval_obs = nullptr;
    float *eval_act = nullptr;   // [2][E][3] ping-pong
    double *eval_reward = nullptr;
    uint8_t *eval_done = nullptr, *eval_complete = nullptr;
    int32_t *eval_host = nullptr;
    int32_t *eval_topology = nullptr;   // the caller's [sum of target][16] buffer (meshenv_eval_set_topology), NULL = detached
};

namespace {

#define HIP_TRY(h, expr)                                                                            \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) {                                                                     \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                           \
            return MESHENV_E_HIP;                                                                   \
        }                                                                                           \
    } while (0)

template <typename T>
int dev_alloc(MeshEnv *h, T **out, size_t count)
{
    void *p = nullptr;
    if (count == 0) count = 1;
    hipError_t e = hipMalloc(&p, count * sizeof(T));
    if (e != hipSuccess) {
        h->err = std::string("hipMalloc: ") + hipGetErrorString(e);
        return MESHENV_E_HIP;
    }
    h->allocs.push_back(p);
    *out = (T *)p;
    return MESHENV_OK;
}

// Every entry point that launches, copies or synchronises runs on the HANDLE's device and leaves the caller's current
// device as it found it (a process may hold handles on several GPUs, and torch tracks its own current device).
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) err = hipSetDevice(device);
        else prev = -1;  // nothing to restore
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define MESHENV_ON_DEVICE(h)              \
    DeviceGuard _guard((h)->device);      \
    HIP_TRY(h, _guard.err)

int fail_arg(MeshEnv *h, const char *msg)
{
    if (h) h->err = msg;
    else g_create_error = msg;
    return MESHENV_E_ARG;
}

// ---- the step kernels, parallel to StepVariant (csrc/meshenv_step_variant.h): the group rows, then the one-wave-per-env rows
using GroupKernel = void (*)(MESHENV_ENTRY_PARAMS GroupArgs);
using WaveKernel = void (*)(KStepArgs);
const GroupKernel kGroupKernels[] = {
    k_step_group<16, true, true, false>, k_step_group<16, true, false, true>, k_step_group<8, true, false, true>,
    k_step_group<16, true, false, false>, k_step_group<8, true, false, false>};
const WaveKernel kWaveKernels[] = {
    k_step<false, true, true, false, false>, k_step<false, false, true, false, false>, k_step<false, true, false, true, true>,
    k_step<false, true, false, false, true>, k_step<false, true, false, true, false>, k_step<false, true, false, false, false>,
    k_step<false, false, false, false, false>,
    k_step<true, true, true, false, false>, k_step<true, false, true, false, false>, k_step<true, true, false, true, false>,
    k_step<true, true, false, false, false>, k_step<true, false, false, false, false>};
static_assert(sizeof(kGroupKernels) / sizeof(kGroupKernels[0]) == kStepGroupVariants &&
                  sizeof(kWaveKernels) / sizeof(kWaveKernels[0]) == kStepWaveVariants,
              "one kernel per StepVariant row");

StepFacts step_facts(const MeshEnv *h, bool multi)
{
    return {multi, h->default_params, h->front_moved, h->group, h->env_lds != nullptr, h->cap, h->stage_bits};
}

// ---- what every handle but MeshEnv derives from: its device, its stream and the text of its *_last_error
struct HandleBase {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
};

template <typename H>
int fail(H *h, int rc, const std::string &msg)
{
    h->err = msg;
    return rc;
}

// The prologue of every *_create: a new H on `device` and `stream` in *out.  `refusal`: what the caller found wrong with its
// own arguments, if anything.  A failed create leaves its message where *_last_error(NULL) reads it.
template <typename H>
int create_handle(const char *fn, int device, void *stream, H **out, const std::string &refusal = std::string())
{
    if (!out) return MESHENV_E_ARG;
    *out = nullptr;
    if (!refusal.empty()) {
        g_create_error = std::string(fn) + ": " + refusal;
        return MESHENV_E_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        g_create_error = std::string(fn) + ": no such HIP device";
        return MESHENV_E_HIP;
    }
    *out = new H();
    (*out)->device = device;
    (*out)->stream = (hipStream_t)stream;
    return MESHENV_OK;
}

// The epilogue of a *_destroy: waits for the handle's stream, frees its one device allocation (or none), deletes it.
template <typename H>
void destroy_handle(H *h, void *buf)
{
    if (!h) return;
    DeviceGuard guard(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (buf) (void)hipFree(buf);
    delete h;
}

int set_stream(HandleBase *h, void *stream)
{
    if (!h) return MESHENV_E_ARG;
    h->stream = (hipStream_t)stream;
    return MESHENV_OK;
}

const char *last_error(const HandleBase *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

// `count` floats at *buf, allocated and zeroed on the first call.  Synchronised: the stream may change before they are read.
bool zeroed_once(const HandleBase *h, float **buf, size_t count)
{
    if (*buf) return true;
    return hipMalloc((void **)buf, count * sizeof(float)) == hipSuccess &&
           hipMemsetAsync(*buf, 0, count * sizeof(float), h->stream) == hipSuccess && hipStreamSynchronize(h->stream) == hipSuccess;
}

// Under the caller's guard of the handle's device: `enqueue` (the hipLaunchKernelGGL of one kernel), then the launch error,
// under fn's name.
template <typename H, typename F>
int launch(H *h, const DeviceGuard &guard, const char *fn, F &&enqueue, const char *what = "launch")
{
    if (guard.err != hipSuccess) return fail(h, MESHENV_E_HIP, std::string(fn) + ": hipSetDevice failed");
    enqueue();
    if (hipGetLastError() != hipSuccess) return fail(h, MESHENV_E_HIP, std::string(fn) + ": " + what + " failed");
    return MESHENV_OK;
}

// ---- what the loss-gradient handles share; csrc/meshenv_grad_bind.h describes their binds
struct GradHandle : HandleBase {
    float *grad = nullptr;      // the caller's flat gradient buffer (the layout's stride floats)
    float *partial = nullptr;   // kCgMaxGroups partial sets, zeroed once
    bool bound = false;
};

// A bind behind its null-handle check: d's refusal of the arguments, then `partial_floats` zeroed floats on the handle's device,
// then grad_dev committed.  The caller commits its tensors after MESHENV_OK: a refused bind leaves the handle as it was.
int grad_bind(GradHandle *g, const GradBind &d, const float *const *const *nets, const int *counts, float *grad_dev, int64_t n_grad,
              int64_t want, size_t partial_floats)
{
    const std::string refusal = grad_bind_refusal(d, nets, counts, grad_dev, n_grad, want);
    if (!refusal.empty()) return fail(g, MESHENV_E_ARG, refusal);
    DeviceGuard guard(g->device);
    if (guard.err != hipSuccess) return fail(g, MESHENV_E_HIP, std::string(d.fn) + ": hipSetDevice failed");
    if (!zeroed_once(g, &g->partial, partial_floats)) return fail(g, MESHENV_E_HIP, std::string(d.fn) + ": allocation failed");
    g->grad = grad_dev;
    g->bound = true;
    return MESHENV_OK;
}

// An optional array of `count` outputs of one kind ("per-sample", "per-row", "activation"): absent, or every entry there.
template <typename H>
int outputs_ok(H *h, const char *fn, float *const *out, int count, const char *kind)
{
    for (int i = 0; out && i < count; i++)
        if (!out[i]) return fail(h, MESHENV_E_ARG, std::string(fn) + ": null " + kind + " output");
    return MESHENV_OK;
}

// The two launches of a backward under the caller's guard: the gradient kernel, then the reduction of its partial sets.
template <typename H, typename F, typename R>
int launch_reduced(H *h, const DeviceGuard &guard, const char *fn, F &&grad_kernel, R &&reduction)
{
    const int rc = launch(h, guard, fn, grad_kernel);
    return rc != MESHENV_OK ? rc : launch(h, guard, fn, reduction, "reduction launch");
}

// The kernels' pointers into `buf`, from consecutive slots of the network's PackLayout (meshenv_pack.h).
void point(const float *buf, const PackSlot *s, std::initializer_list<const float **> ptrs)
{
    for (const float **p : ptrs) *p = buf + (s++)->off;
}

// The launch of every *_refresh: one k_target_pack over the live tensors that the handle's *_bind put into its table by the
// network's PackLayout, the description its buffer was packed by.
template <typename H>
int pack_refresh(H *h, const char *fn)
{
    DeviceGuard guard(h->device);
    return launch(h, guard, fn, [&] {
        hipLaunchKernelGGL(k_target_pack, dim3(pack_blocks(h->table, h->n_copies), h->n_copies), dim3(256), 0, h->stream, h->table);
    });
}

}  // namespace

// ---- the handle of DDPG's gradient statements (include/meshenv_ddpg_grad.h) and what its entry points call under their guard
struct MeshDdpgGrad : HandleBase {
    WgNet a{}, c{};              // the live actor and critic
    float *grad = nullptr;       // the caller's flat gradient buffer: the actor's set, then the critic's
    float *space = nullptr;      // rows_cap rows of kWgRowFloats, then the partial tiles of the chunks
    int rows_cap = 0;            // the largest n seen, rounded up to 16
    float loss_scale = 1.0f;
    bool bound = false;
};

namespace {

int wg_rows16(int n) { return (n + kCgRows - 1) / kCgRows * kCgRows; }

// the most chunks a call of at most rows16 rows has
int wg_chunks_cap(int rows16)
{
    const int c = (rows16 / kCgRows + kWgMinChunkTiles - 1) / kWgMinChunkTiles;
    return c < kWgMaxChunks ? c : kWgMaxChunks;
}

// The workspace for n rows: grows only, and waits for the handle's stream before the old one is freed
int wg_reserve(MeshDdpgGrad *g, int n, const char *fn)
{
    const int rows16 = wg_rows16(n);
    if (rows16 <= g->rows_cap) return MESHENV_OK;
    if (hipStreamSynchronize(g->stream) != hipSuccess) return fail(g, MESHENV_E_HIP, std::string(fn) + ": hipStreamSynchronize failed");
    if (g->space) (void)hipFree(g->space);
    g->space = nullptr;
    g->rows_cap = 0;
    const size_t floats = (size_t)rows16 * kWgRowFloats + (size_t)wg_chunks_cap(rows16) * kWgJobs * 256;
    if (hipMalloc((void **)&g->space, floats * sizeof(float)) != hipSuccess) {
        g->space = nullptr;
        return fail(g, MESHENV_E_HIP, std::string(fn) + ": allocation of the workspace failed");
    }
    g->rows_cap = rows16;
    return MESHENV_OK;
}

// the matrices of a call of rows16 rows in the workspace (16-byte aligned: every stride is a multiple of 4 floats)
WgSpace wg_space(const MeshDdpgGrad *g, int rows16, float **partial)
{
    WgSpace s;
    float *p = g->space;
    const size_t r = (size_t)rows16;
    s.x0 = p;  p += r * kWgX0;
    s.a1 = p;  p += r * kWgA1;
    s.a2 = p;  p += r * kWgA2;
    s.dz1 = p; p += r * kWgH1;
    s.dz2 = p; p += r * kWgH2Pad;
    s.dh = p;
    *partial = g->space + (size_t)g->rows_cap * kWgRowFloats;
    return s;
}

// phase B and the ordered reduction of either statement
template <int KIN, int NOUT>
int wg_weights(MeshDdpgGrad *g, const DeviceGuard &guard, const char *fn, const WgSpace &ws, float *partial, int n, float scale,
               float *grad, float *loss_dev)
{
    const int rows16 = wg_rows16(n), chunk_rows = kCgRows * wg_chunk_tiles(n), chunks = (rows16 + chunk_rows - 1) / chunk_rows;
    const int rc = launch(g, guard, fn, [&] {
        hipLaunchKernelGGL(k_wgrad_weights, dim3(kWgJobs / kWgJobWaves, chunks), dim3(64 * kWgJobWaves), 0, g->stream, ws, rows16,
                           chunk_rows, partial);
    }, "weight phase launch");
    if (rc != MESHENV_OK) return rc;
    return launch(g, guard, fn, [&] {
        hipLaunchKernelGGL((k_wgrad_reduce<KIN, NOUT>), dim3(kWgJobs), dim3(256), 0, g->stream, (const float *)partial, chunks, n, scale,
                           grad, loss_dev);
    }, "reduction launch");
}

}  // namespace

extern "C" {

void meshenv_default_params(MeshEnvParams *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(MeshEnvParams);
    p->neighbor_num = 6;
    p->radius_num = 3;
    p->fail_limit = 100;
    p->log_capacity = 0;
    p->radius = kDefRadius;
    p->max_ref_angle = kDefMaxRefAngle;
    p->key_lambda = kDefKeyLambda;
    p->min_degree = kDefMinDegree;
    p->max_degree = kDefMaxDegree;
    p->same_point_eps = kDefSameEps;
    p->ray_length = kDefRayLength;
}

int meshenv_abi_version(void) { return MESHENV_ABI_VERSION; }

int meshenv_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *meshenv_last_error(const MeshEnv *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

void meshenv_destroy(MeshEnv *h)
{
    if (!h) return;
    DeviceGuard guard(h->device);
    (void)hipStreamSynchronize(h->stream);
    for (void *p : h->allocs) (void)hipFree(p);
    if (h->eval_host) (void)hipHostFree(h->eval_host);
    for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    delete h;
}

}  // extern "C"

// shared body of meshenv_create (domains from host arrays) and meshenv_create_random (gen != NULL: the rings and their
// constants are produced on the device, csrc/meshenv_domgen.h; dom_xy_host / dom_consts_host are NULL then)
static int create_impl(int device, int n_domains, const int32_t *dom_offsets_host, const double *dom_xy_host,
                       const double *dom_consts_host, int n_envs, const int32_t *env_domain_host,
                       const MeshEnvParams *params, void *stream, const GenParams *gen, MeshEnv **out)
{
    if (!out) return fail_arg(nullptr, "meshenv_create: out is NULL");
    *out = nullptr;
    if (n_domains <= 0 || n_envs <= 0 || !dom_offsets_host || !env_domain_host || (!gen && (!dom_xy_host || !dom_consts_host)))
        return fail_arg(nullptr, "meshenv_create: null or empty input");
    MeshEnvParams prm;
    meshenv_default_params(&prm);
    if (params) {
        if (params->struct_size != (int32_t)sizeof(MeshEnvParams))
            return fail_arg(nullptr, "meshenv_create: MeshEnvParams.struct_size mismatch (ABI)");
        prm = *params;
    }
    if (prm.neighbor_num != 6 || prm.radius_num != 3)
        return fail_arg(nullptr, "meshenv_create: neighbor_num must be 6 and radius_num 3 (observation layout)");
    if (prm.fail_limit <= 0 || prm.log_capacity < 0 || !(prm.radius > 0))
        return fail_arg(nullptr, "meshenv_create: bad parameter value");

    int max_ring = 0;
    for (int d = 0; d < n_domains; d++) {
        const int n0 = dom_offsets_host[d + 1] - dom_offsets_host[d];
        if (n0 < 4) return fail_arg(nullptr, "meshenv_create: a domain ring needs at least 4 vertices");
        max_ring = n0 > max_ring ? n0 : max_ring;
        if (gen) continue;
        // Domains on which the reference divides by zero (supported coordinate range): a zero area
        // (current_area / original_area, rl/boundary_env.py) and a base length -- the mean of the six edges around a
        // vertex rounded to 4 places (general/components.py) -- that rounds to 0 (observation = distance / base length).
        const double area = dom_consts_host[3 * d];
        if (!(area != 0.0) || !std::isfinite(area))
            return fail_arg(nullptr, "meshenv_create: a domain's area is 0 or not finite (the reference divides by it; "
                                     "far from the origin a small domain's shoelace area cancels)");
        const double *xy = dom_xy_host + 2 * (size_t)dom_offsets_host[d];
        for (int i = 0; i < 2 * n0; i++)
            if (!(std::fabs(xy[i]) < 1e100))
                return fail_arg(nullptr, "meshenv_create: a domain coordinate is not finite or not below 1e100 in magnitude");
        auto edge = [&](int i) {   // length of edge (i, i + 1), indices mod n0
            const int a = ((i % n0) + n0) % n0, b = (a + 1) % n0;
            const double dx = xy[2 * a] - xy[2 * b], dy = xy[2 * a + 1] - xy[2 * b + 1];
            return std::sqrt(dx * dx + dy * dy);
        };
        for (int i = 0; i < n0; i++) {
            double sum = 0;
            for (int k = -3; k < 3; k++) sum += edge(i + k);
            if (!((sum / 6) * 1e4 > 0.5))
                return fail_arg(nullptr, "meshenv_create: a domain's base length (mean of six consecutive edges) rounds "
                                         "to 0 at 4 places (edges below 5e-5: the reference divides by it)");
        }
    }
    for (int e = 0; e < n_envs; e++)
        if (env_domain_host[e] < 0 || env_domain_host[e] >= n_domains)
            return fail_arg(nullptr, "meshenv_create: env_domain entry out of range");
    const int cap = (max_ring + 15) / 16 * 16;
    const size_t lds = lds_bytes_for(cap);
    if (lds > 160 * 1024) return fail_arg(nullptr, "meshenv_create: ring too long for one CU's LDS (160 KB: about 3600 vertices)");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        g_create_error = "meshenv_create: no HIP device available (this library has no CPU fallback)";
        return MESHENV_E_HIP;
    }
    if (device < 0 || device >= ndev) return fail_arg(nullptr, "meshenv_create: device index out of range");

    MeshEnv *h = new MeshEnv();
    h->device = device;
    h->stream = (hipStream_t)stream;
    h->n_envs = n_envs;
    h->n_domains = n_domains;
    h->cap = cap;
    h->max_ring = max_ring;
    h->lds = lds;
#define CREATE_TRY(expr)                                            \
    do {                                                            \
        int _rc = (expr);                                           \
        if (_rc != MESHENV_OK) {                                    \
            g_create_error = h->err;                                \
            meshenv_destroy(h);                                     \
            return _rc;                                             \
        }                                                           \
    } while (0)
#define CREATE_HIP(expr)                                                                \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) {                                                         \
            g_create_error = std::string(#expr) + ": " + hipGetErrorString(_e);         \
            meshenv_destroy(h);                                                         \
            return MESHENV_E_HIP;                                                       \
        }                                                                               \
    } while (0)

    DeviceGuard guard(device);
    CREATE_HIP(guard.err);
    // The attribute is per function, not per handle: always raise it to the CU's full 160 KB so that a later handle with
    // shorter rings cannot lower the cap under an earlier one.
    constexpr int kLdsCap = 160 * 1024;
    if (lds > 64 * 1024) {
        for (int v = kStepGroupVariants; v < kStepVariantCount; v++)   // every k_step that can meet rings of more than 64 slots
            if (!kStepVariants[v].small)
                CREATE_HIP(hipFuncSetAttribute((const void *)kWaveKernels[v - kStepGroupVariants], hipFuncAttributeMaxDynamicSharedMemorySize, kLdsCap));
        CREATE_HIP(hipFuncSetAttribute((const void *)k_reset, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsCap));
        CREATE_HIP(hipFuncSetAttribute((const void *)k_init_domains, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsCap));
    }
    CREATE_HIP(upload_atan_state());   // the tie-breaker of every quantised angle (csrc/meshenv_geom.h, atan2_nc)

    // Single-step kernel variant.  The CU-group kernel (G envs per workgroup, SIMD-balanced updates) pays off in the
    // latency-bound regime only: one workgroup per CU (n_envs <= 256 * G) with G >= 8; measured on MI355X,
    // boundary(): 4096 envs 20.2 -> 19.4 us/step (G = 16), 2048 envs 16.5 -> 16.0 (G = 8), but 8192 envs
    // 25.0 -> 34.6 and 65536 envs 103 -> 231 us/step, where throughput, not the slowest wave, sets the time.
    {
        int n_cu = 256;  // MI355X; read from the device so that a partitioned GPU (CPX / fewer CUs) keeps one workgroup per CU
        CREATE_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
        if (n_cu <= 0) n_cu = 256;
        h->n_cu = n_cu;
        int G = 1;
        const char *force = getenv("MESHENV_GROUP");
        int want = 1;
        if (force) want = atoi(force);
        else if (n_envs <= n_cu * 16) {
            int g = 1;
            while (g * 2 <= n_envs / n_cu && g * 2 <= 16) g *= 2;
            want = g >= 8 ? g : 1;
        }
        for (int g : {16, 8})
            if (g <= want && group_lds_bytes(cap, g) <= 150 * 1024) { G = g; break; }
        if (!force && (G < 8 || n_envs > n_cu * G)) G = 1;  // LDS forced a smaller group: more than one workgroup per CU
        // Ragged packing: sixteen rings of the LONGEST stride do not fit, sixteen rings of their own lengths may (mixed
        // d1 / d2 / d3: 120 / 196 / 272 vertices -> 135 KB instead of 197 KB).  One workgroup per CU as in the uniform case.
        // (MESHENV_GROUP=16 asks for sixteen: the packing is tried before the batch settles for eight rings of the longest stride)
        if ((G == 1 || (force && G < 16)) && want == 16 && n_envs <= n_cu * 16 && group_lds_bytes(cap, 16) > 150 * 1024) {
            std::vector<int2> pack((size_t)n_envs);
            size_t worst = 0;
            for (int w0 = 0; w0 < n_envs; w0 += 16) {
                size_t off = 0;
                for (int e = w0; e < w0 + 16 && e < n_envs; e++) {
                    const int d = env_domain_host[e];
                    const int n0 = dom_offsets_host[d + 1] - dom_offsets_host[d];
                    const int cap_e = (n0 + 15) / 16 * 16;
                    pack[(size_t)e] = make_int2((int)off, cap_e);
                    off += lds_bytes_for(cap_e);
                }
                worst = off > worst ? off : worst;
            }
            worst = (worst + 31) / 32 * 32;
            if (worst + 16 * sizeof(Handoff) <= (size_t)kLdsCap) {   // one workgroup per CU: the whole 160 KB may go to it
                G = 16;
                h->env_lds_host.swap(pack);
                h->ho_off = (int)worst;
            }
        }
        MeshEnvParams def;
        meshenv_default_params(&def);
        h->default_params = prm.radius == def.radius && prm.max_ref_angle == def.max_ref_angle && prm.key_lambda == def.key_lambda &&
                            prm.min_degree == def.min_degree && prm.max_degree == def.max_degree &&
                            prm.same_point_eps == def.same_point_eps && prm.ray_length == def.ray_length;
        if (!h->default_params) G = 1;  // the group kernels exist with literal (default) geometry constants only
        if (!h->default_params) h->env_lds_host.clear();
        h->group = G;
        h->group_lds = h->env_lds_host.empty() ? group_lds_bytes(cap, G) : (size_t)h->ho_off + 16 * sizeof(Handoff);
        // staging mode of the one-wave-per-env step kernel (bits 1, 2 of its auto_reset argument), decided once per handle:
        // record-first staging (memoised rejections never load their ring) -- measured never slower from 8192 envs up,
        // +9..15 % at 32 768+; the ring staged without candidate keys / stamps -- +0..3 % from 32 768 envs, -2 % at 8192.
        // MESHENV_LAZY / MESHENV_LIGHT override the size rule (A/B switches, read here, not per launch).
        {
            const char *lz = getenv("MESHENV_LAZY");
            const bool lazy = lz ? atoi(lz) != 0 : n_envs >= 8192;
            const char *lt = getenv("MESHENV_LIGHT");
            const bool light = lt ? atoi(lt) != 0 : (lazy && n_envs >= 16384);
            h->stage_bits = (lazy ? 2 : 0) | (light ? 4 : 0);
        }
    }

    DevState &S = h->S;
    S.n_domains = n_domains;
    S.n_envs = n_envs;
    S.prm.radius = prm.radius;
    S.prm.max_ref_angle = prm.max_ref_angle;
    S.prm.w0 = prm.key_lambda;
    S.prm.w1 = 1 - prm.key_lambda;
    S.prm.min_degree = prm.min_degree;
    S.prm.max_degree = prm.max_degree;
    S.prm.same_eps = prm.same_point_eps;
    S.prm.ray_length = prm.ray_length;
    S.prm.fail_limit = prm.fail_limit;
    S.prm.log_cap = prm.log_capacity;

    const int total_dom = dom_offsets_host[n_domains];
    h->dom_off_host.assign(dom_offsets_host, dom_offsets_host + n_domains + 1);
    h->env_dom_host.assign(env_domain_host, env_domain_host + n_envs);
    const size_t total_env = (size_t)n_envs * (size_t)cap;  // uniform ring stride
    S.cap = cap;

    double2 *d_dom_xy = nullptr;
    DevCold &K = h->cold;  // host copy of the rarely used pointers; the kernels read the device copy S.cold
    std::memset(&K, 0, sizeof(K));
    CREATE_TRY(dev_alloc(h, &S.dom, (size_t)n_domains));
    CREATE_TRY(dev_alloc(h, &d_dom_xy, (size_t)total_dom));
    CREATE_TRY(dev_alloc(h, &K.dom_key, (size_t)total_dom));
    CREATE_TRY(dev_alloc(h, &K.dom_stamp, (size_t)total_dom));
    CREATE_TRY(dev_alloc(h, &K.dom_obs, (size_t)n_domains * kObsDim));
    CREATE_TRY(dev_alloc(h, &S.ring_xy, total_env));
    CREATE_TRY(dev_alloc(h, &S.ring_id, total_env));
    CREATE_TRY(dev_alloc(h, &S.ring_key, total_env));
    CREATE_TRY(dev_alloc(h, &S.ring_stamp, total_env));
    CREATE_TRY(dev_alloc(h, &S.scal, (size_t)n_envs));
    CREATE_TRY(dev_alloc(h, &S.cnt, (size_t)n_envs));
    CREATE_TRY(dev_alloc(h, &S.obs_cache, (size_t)n_envs * kObsDim));
    if (!h->env_lds_host.empty()) {
        CREATE_TRY(dev_alloc(h, &h->env_lds, (size_t)n_envs));
        CREATE_HIP(hipMemcpy(h->env_lds, h->env_lds_host.data(), sizeof(int2) * (size_t)n_envs, hipMemcpyHostToDevice));
    }
    if (h->group > 1 && h->group_lds > 64 * 1024)   // the one CU-group kernel this handle steps with (env_lds decides ragged)
        CREATE_HIP(hipFuncSetAttribute((const void *)kGroupKernels[select_step_variant(step_facts(h, false))], hipFuncAttributeMaxDynamicSharedMemorySize, kLdsCap));
    if (prm.log_capacity > 0) {
        CREATE_TRY(dev_alloc(h, &K.log_quads, (size_t)n_envs * 2 * prm.log_capacity * 4));
        CREATE_TRY(dev_alloc(h, &K.log_vxy, (size_t)n_envs * 2 * prm.log_capacity));
        CREATE_TRY(dev_alloc(h, &K.last_ep, (size_t)n_envs));
        CREATE_HIP(hipMemsetAsync(K.last_ep, 0, sizeof(LastEpisode) * (size_t)n_envs, h->stream));
    }
    K.dom_xy = d_dom_xy;
    {
        DevCold *cold_dev = nullptr;
        CREATE_TRY(dev_alloc(h, &cold_dev, (size_t)1));
        CREATE_HIP(hipMemcpy(cold_dev, &K, sizeof(DevCold), hipMemcpyHostToDevice));
        S.cold = cold_dev;
    }
#ifdef MESHENV_STAMPS
    CREATE_TRY(dev_alloc(h, &S.dbg, (size_t)n_envs * 16));
#endif

    std::vector<EnvScalars> sc((size_t)n_envs);
    std::memset(sc.data(), 0, sc.size() * sizeof(EnvScalars));
    for (int e = 0; e < n_envs; e++) sc[e].dom = env_domain_host[e];

    if (!gen) {
        std::vector<DomConst> dc((size_t)n_domains);
        std::memset(dc.data(), 0, dc.size() * sizeof(DomConst));
        for (int d = 0; d < n_domains; d++) {
            dc[d].orig_area = dom_consts_host[3 * d];
            dc[d].min_area = dom_consts_host[3 * d + 1] * dom_consts_host[3 * d + 1];   // estimated_area_range[0] ** 2
            dc[d].crit_area = dom_consts_host[3 * d + 2] * dom_consts_host[3 * d + 2];  // estimated_area_range[1] ** 2
            dc[d].off = dom_offsets_host[d];
            dc[d].n0 = dom_offsets_host[d + 1] - dom_offsets_host[d];
            dc[d].ref = -1;
        }
        CREATE_HIP(hipMemcpy(S.dom, dc.data(), sizeof(DomConst) * (size_t)n_domains, hipMemcpyHostToDevice));
        CREATE_HIP(hipMemcpy(d_dom_xy, dom_xy_host, sizeof(double2) * (size_t)total_dom, hipMemcpyHostToDevice));
    } else {
        // the rings at their offsets, then the constants: two launches, nothing generated on the host
        int32_t *d_off = nullptr;
        int *d_err = nullptr;
        CREATE_TRY(dev_alloc(h, &d_off, (size_t)n_domains + 1));
        CREATE_TRY(dev_alloc(h, &d_err, (size_t)1));
        CREATE_HIP(hipMemcpy(d_off, dom_offsets_host, sizeof(int32_t) * ((size_t)n_domains + 1), hipMemcpyHostToDevice));
        CREATE_HIP(hipMemset(d_err, 0, sizeof(int)));
        if (gen->density_mode)
            hipLaunchKernelGGL(k_gen_rings_density, dim3(n_domains), dim3(64), 0, h->stream, *gen, n_domains, (const int32_t *)d_off, d_dom_xy, d_err);
        else
            hipLaunchKernelGGL(k_gen_rings, dim3(n_domains), dim3(64), 0, h->stream, *gen, n_domains, (const int32_t *)d_off, d_dom_xy, d_err);
        CREATE_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_dom_consts, dim3(n_domains), dim3(64), sizeof(double2) * (size_t)max_ring, h->stream, n_domains,
                           (const int32_t *)d_off, (const double2 *)d_dom_xy, S.dom);
        CREATE_HIP(hipGetLastError());
        int err = 0;
        CREATE_HIP(hipMemcpy(&err, d_err, sizeof(int), hipMemcpyDeviceToHost));
        if (err) {
            g_create_error = "meshenv_create_random: a ring could not be generated on the device (fewer than 5 distinct pixels, or a length mismatch between the two passes)";
            meshenv_destroy(h);
            return MESHENV_E_STATE;
        }
    }
    CREATE_HIP(hipMemcpy(S.scal, sc.data(), sizeof(EnvScalars) * (size_t)n_envs, hipMemcpyHostToDevice));
    CREATE_HIP(hipMemset(S.ring_xy, 0, sizeof(double2) * total_env));
    CREATE_HIP(hipMemset(S.ring_id, 0, sizeof(int32_t) * total_env));
    CREATE_HIP(hipMemset(S.ring_key, 0, sizeof(double) * total_env));
    CREATE_HIP(hipMemset(S.ring_stamp, 0, sizeof(int32_t) * total_env));

    hipLaunchKernelGGL(k_init_domains, dim3(n_domains), dim3(64), lds, h->stream, S, cap);
    CREATE_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_reset, dim3(n_envs), dim3(64), lds, h->stream, S, cap, (const uint8_t *)nullptr, (float *)nullptr, 1, 0ULL,
                       0, (int32_t *)nullptr, (int32_t *)nullptr);
    CREATE_HIP(hipGetLastError());
    CREATE_HIP(hipStreamSynchronize(h->stream));
#undef CREATE_TRY
#undef CREATE_HIP
    *out = h;
    return MESHENV_OK;
}

extern "C" {

int meshenv_create(int device, int n_domains, const int32_t *dom_offsets_host, const double *dom_xy_host,
                   const double *dom_consts_host, int n_envs, const int32_t *env_domain_host,
                   const MeshEnvParams *params, void *stream, MeshEnv **out)
{
    return create_impl(device, n_domains, dom_offsets_host, dom_xy_host, dom_consts_host, n_envs, env_domain_host, params,
                       stream, nullptr, out);
}

// clockwise_angle(a, b) of ui/tk-ui.py:185-192 and its cosine / sine for the offset (dx, dy) = b - a: the host libm's
// values -- the reference's -- in the reference's expression order (domains.clockwise_angle).  integer: the coordinates
// are Python ints, so -(b[1] - a[1]) of a zero difference is the int 0, i.e. +0.0 in atan2 (a float difference gives -0.0).
static void edge_direction(double dx, double dy, bool integer, double *cs)
{
    volatile double ny = (integer && dy == 0) ? 0.0 : -dy, x = dx;   // volatile: the calls must reach the running libm
    const double theta = -std::atan2(ny, x);
    volatile double angle = std::copysign(1.0, theta) >= 0 ? theta : 2 * 3.141592653589793 + theta;
    cs[0] = std::cos(angle);
    cs[1] = std::sin(angle);
}

// shared by meshenv_create_random (uniform split) and meshenv_create_random_density (calculate_density)
static int create_random_impl(const char *fn, int device, int n_envs, GenParams gp, const uint64_t *seeds_host,
                              const MeshEnvParams *params, void *stream, MeshEnv **out, uint8_t *raises_host)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        g_create_error = std::string(fn) + ": no HIP device available (this library has no CPU fallback)";
        return MESHENV_E_HIP;
    }
    if (device < 0 || device >= ndev) return fail_arg(nullptr, "meshenv_create_random: device index out of range");
    // pass 1: the ring lengths (the domain table and the ring stride are sized from them)
    std::vector<int32_t> offs((size_t)n_envs + 1, 0), env_dom((size_t)n_envs);
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) { g_create_error = std::string(fn) + ": hipSetDevice failed"; return MESHENV_E_HIP; }
    int32_t *d_cnt = nullptr;
    int *d_err = nullptr;
    unsigned long long *d_seeds = nullptr;
    double2 *d_tab = nullptr;
    unsigned char *d_raises = nullptr;
    auto cleanup = [&]() {
        if (d_cnt) (void)hipFree(d_cnt);
        if (d_err) (void)hipFree(d_err);
        if (d_seeds) (void)hipFree(d_seeds);
        if (d_tab) (void)hipFree(d_tab);
        if (d_raises) (void)hipFree(d_raises);
    };
    bool ok = hipMalloc((void **)&d_cnt, sizeof(int32_t) * (size_t)n_envs) == hipSuccess &&
              hipMalloc((void **)&d_err, sizeof(int)) == hipSuccess && hipMemset(d_err, 0, sizeof(int)) == hipSuccess;
    if (ok && seeds_host) {
        ok = hipMalloc((void **)&d_seeds, sizeof(unsigned long long) * (size_t)n_envs) == hipSuccess &&
             hipMemcpy(d_seeds, seeds_host, sizeof(unsigned long long) * (size_t)n_envs, hipMemcpyHostToDevice) == hipSuccess;
        gp.seeds = d_seeds;
    }
    if (ok && gp.density_mode) {
        // pixel coordinates lie in ctr -+ 2 aveRadius (radii are clipped to [0, 2 aveRadius]): offsets within 4 aveRadius + 1
        const int R = (int)std::ceil(4 * gp.ave_radius) + 1, W = 2 * R + 1;
        std::vector<double> tab((size_t)W * W * 2);
        for (int dx = -R; dx <= R; dx++)
            for (int dy = -R; dy <= R; dy++) edge_direction((double)dx, (double)dy, true, &tab[((size_t)(dx + R) * W + (dy + R)) * 2]);
        ok = hipMalloc((void **)&d_tab, sizeof(double2) * (size_t)W * W) == hipSuccess &&
             hipMemcpy(d_tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice) == hipSuccess &&
             hipMalloc((void **)&d_raises, (size_t)n_envs) == hipSuccess && hipMemset(d_raises, 0, (size_t)n_envs) == hipSuccess;
        gp.dir_tab = d_tab;
        gp.dir_r = R;
        gp.raises = d_raises;
    }
    int err = 0;
    if (ok) {
        if (gp.density_mode) hipLaunchKernelGGL(k_gen_count_density, dim3(n_envs), dim3(64), 0, (hipStream_t)stream, gp, n_envs, d_cnt, d_err);
        else hipLaunchKernelGGL(k_gen_count, dim3(n_envs), dim3(64), 0, (hipStream_t)stream, gp, n_envs, d_cnt, d_err);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize((hipStream_t)stream) == hipSuccess &&
             hipMemcpy(offs.data() + 1, d_cnt, sizeof(int32_t) * (size_t)n_envs, hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(&err, d_err, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
    }
    int n_raise = 0;
    if (ok && gp.density_mode) {
        std::vector<uint8_t> rz((size_t)n_envs);
        ok = hipMemcpy(rz.data(), d_raises, (size_t)n_envs, hipMemcpyDeviceToHost) == hipSuccess;
        for (int k = 0; k < n_envs; k++) n_raise += rz[(size_t)k] ? 1 : 0;
        if (raises_host) std::memcpy(raises_host, rz.data(), (size_t)n_envs);
    }
    if (!ok) { cleanup(); g_create_error = std::string(fn) + ": the ring-length pass failed (HIP error)"; return MESHENV_E_HIP; }
    if (err) {
        cleanup();
        g_create_error = std::string(fn) + ": a ring could not be generated on the device (fewer than 5 distinct pixels, or a densified ring beyond 2048 points)";
        return MESHENV_E_STATE;
    }
    if (n_raise) {
        cleanup();
        g_create_error = std::string(fn) + ": " + std::to_string(n_raise) + " of " + std::to_string(n_envs) +
                         " polygons have no ring here -- raises_host[k] = 1: calculate_density raises ZeroDivisionError (an edge of "
                         "0.5 - 1.5 spacings, ui/tk-ui.py:263-264); 2: not generated on the device (fewer than 5 distinct pixels, a "
                         "densified ring beyond 2048 points, an edge outside the direction table) -- pass seeds without them";
        return MESHENV_E_STATE;
    }
    if (!out) { cleanup(); return MESHENV_OK; }   // probe only
    for (int k = 0; k < n_envs; k++) {
        if (offs[(size_t)k + 1] < 4) { cleanup(); g_create_error = std::string(fn) + ": empty ring"; return MESHENV_E_STATE; }
        offs[(size_t)k + 1] += offs[(size_t)k];
        env_dom[(size_t)k] = k;
    }
    gp.raises = nullptr;   // pass 2 runs on rings that do not raise
    const int rc = create_impl(device, n_envs, offs.data(), nullptr, nullptr, n_envs, env_dom.data(), params, stream, &gp, out);
    cleanup();
    return rc;
}

static GenParams default_gen_params(uint64_t seed0, int num_verts)
{
    GenParams gp;
    std::memset(&gp, 0, sizeof(gp));
    gp.seed0 = seed0;
    gp.ctr_x = 250; gp.ctr_y = 250; gp.ave_radius = 100; gp.irregularity = 0.55; gp.spikeyness = 0.7;  // GenerateRandomPolygon.py:63
    gp.fixed_verts = num_verts;
    return gp;
}

int meshenv_create_random(int device, int n_envs, uint64_t seed0, int num_verts, double edge, const MeshEnvParams *params,
                          void *stream, MeshEnv **out)
{
    if (!out) return fail_arg(nullptr, "meshenv_create_random: out is NULL");
    *out = nullptr;
    if (n_envs <= 0 || !(edge > 0.0) || num_verts < 0 || (num_verts > 0 && (num_verts < 5 || num_verts > kGenMaxVerts)))
        return fail_arg(nullptr, "meshenv_create_random: n_envs > 0, edge > 0 and num_verts in {0, 5..64} are required");
    GenParams gp = default_gen_params(seed0, num_verts);
    gp.edge = edge;
    return create_random_impl("meshenv_create_random", device, n_envs, gp, nullptr, params, stream, out, nullptr);
}

int meshenv_create_random_density(int device, int n_envs, uint64_t seed0, const uint64_t *seeds_host, int num_verts,
                                  double base_length, double density, const MeshEnvParams *params, void *stream, MeshEnv **out,
                                  uint8_t *raises_host)
{
    if (out) *out = nullptr;
    if (n_envs <= 0 || !(base_length > 0.0) || !(density > 0.0) || num_verts < 0 ||
        (num_verts > 0 && (num_verts < 5 || num_verts > kGenMaxVerts)))
        return fail_arg(nullptr, "meshenv_create_random_density: n_envs > 0, base_length > 0, density > 0 and num_verts in {0, 5..64} are required");
    GenParams gp = default_gen_params(seed0, num_verts);
    gp.density_mode = 1;
    gp.base_length = base_length;
    gp.density = density;
    return create_random_impl("meshenv_create_random_density", device, n_envs, gp, seeds_host, params, stream, out, raises_host);
}

int meshenv_density_rings(int device, int n_polys, const int32_t *poly_offsets_host, const double *pixels_host, int integer_pixels,
                          const double *densities_host, double base_length, int32_t *count_host, uint8_t *status_host,
                          double *xy_host, int64_t cap_points)
{
    if (n_polys <= 0 || !poly_offsets_host || !pixels_host || !count_host || !status_host || !(base_length > 0.0))
        return MESHENV_E_ARG;
    const int total_in = poly_offsets_host[n_polys];
    for (int k = 0; k < n_polys; k++) {
        const int nv = poly_offsets_host[k + 1] - poly_offsets_host[k];
        if (nv < 3 || nv > kDensMaxVerts) return MESHENV_E_ARG;
    }
    if (integer_pixels)
        for (int i = 0; i < 2 * total_in; i++)
            if (pixels_host[i] != std::floor(pixels_host[i]) || std::fabs(pixels_host[i]) > 1e9) return MESHENV_E_ARG;
    // Edge directions and lengths from the host libm.  The device deduplicates repeated pixels (the reference's dict), so
    // the edge INTO deduplicated vertex r is computed here for the same deduplicated list.
    std::vector<double> dir((size_t)total_in * 2, 0.0), len((size_t)total_in, 0.0);
    volatile double two = 2.0;
    for (int k = 0; k < n_polys; k++) {
        const int o = poly_offsets_host[k], nv = poly_offsets_host[k + 1] - o;
        const double *P = pixels_host + 2 * (size_t)o;
        std::vector<int> keep;
        for (int i = 0; i < nv; i++) {
            bool first = true;
            for (int j = 0; j < i && first; j++) first = !(P[2 * j] == P[2 * i] && P[2 * j + 1] == P[2 * i + 1]);
            if (first) keep.push_back(i);
        }
        const int m = (int)keep.size();
        for (int r = 0; r < m; r++) {
            const int i = keep[(size_t)r], ip = keep[(size_t)(r == 0 ? m - 1 : r - 1)];
            const double dx = P[2 * i] - P[2 * ip], dy = P[2 * i + 1] - P[2 * ip + 1];
            edge_direction(dx, dy, integer_pixels != 0, &dir[2 * (size_t)(o + r)]);
            // distance(): math.sqrt((p1[0] - p2[0]) ** 2 + (p1[1] - p2[1]) ** 2) -- exact int arithmetic for Python ints,
            // libm pow for floats
            len[(size_t)(o + r)] = integer_pixels ? std::sqrt(dx * dx + dy * dy) : std::sqrt(std::pow(-dx, two) + std::pow(-dy, two));
        }
    }
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return MESHENV_E_HIP;
    int32_t *d_off = nullptr, *d_cnt = nullptr, *d_ooff = nullptr;
    double *d_dens = nullptr, *d_px = nullptr, *d_len = nullptr;
    double2 *d_dir = nullptr, *d_out = nullptr;
    unsigned char *d_st = nullptr;
    int rc = MESHENV_OK;
    auto H = [&](hipError_t e) { if (e != hipSuccess && rc == MESHENV_OK) rc = MESHENV_E_HIP; return e == hipSuccess; };
    H(hipMalloc((void **)&d_off, sizeof(int32_t) * ((size_t)n_polys + 1)));
    H(hipMalloc((void **)&d_px, sizeof(double) * 2 * (size_t)total_in));
    H(hipMalloc((void **)&d_cnt, sizeof(int32_t) * (size_t)n_polys));
    H(hipMalloc((void **)&d_ooff, sizeof(int32_t) * ((size_t)n_polys + 1)));
    H(hipMalloc((void **)&d_dir, sizeof(double2) * (size_t)total_in));
    H(hipMalloc((void **)&d_len, sizeof(double) * (size_t)total_in));
    H(hipMalloc((void **)&d_st, (size_t)n_polys));
    if (densities_host) H(hipMalloc((void **)&d_dens, sizeof(double) * (size_t)total_in));
    if (rc == MESHENV_OK) {
        H(hipMemcpy(d_off, poly_offsets_host, sizeof(int32_t) * ((size_t)n_polys + 1), hipMemcpyHostToDevice));
        H(hipMemcpy(d_px, pixels_host, sizeof(double) * 2 * (size_t)total_in, hipMemcpyHostToDevice));
        H(hipMemcpy(d_dir, dir.data(), sizeof(double) * dir.size(), hipMemcpyHostToDevice));
        H(hipMemcpy(d_len, len.data(), sizeof(double) * len.size(), hipMemcpyHostToDevice));
        if (densities_host) H(hipMemcpy(d_dens, densities_host, sizeof(double) * (size_t)total_in, hipMemcpyHostToDevice));
    }
    std::vector<int32_t> ooff((size_t)n_polys + 1, 0);
    if (rc == MESHENV_OK) {
        hipLaunchKernelGGL(k_density_rings<false>, dim3(n_polys), dim3(64), 0, nullptr, n_polys, (const int32_t *)d_off, (const double *)d_px,
                           (const double *)d_dens, (const double2 *)d_dir, (const double *)d_len, base_length, (const int32_t *)nullptr,
                           (double2 *)nullptr, d_cnt, d_st);
        H(hipGetLastError());
        H(hipDeviceSynchronize());
        H(hipMemcpy(count_host, d_cnt, sizeof(int32_t) * (size_t)n_polys, hipMemcpyDeviceToHost));
        H(hipMemcpy(status_host, d_st, (size_t)n_polys, hipMemcpyDeviceToHost));
    }
    if (rc == MESHENV_OK && xy_host) {
        for (int k = 0; k < n_polys; k++) ooff[(size_t)k + 1] = ooff[(size_t)k] + (status_host[k] == 0 ? count_host[k] : 0);
        const int64_t total_out = ooff[(size_t)n_polys];
        if (total_out > cap_points) rc = MESHENV_E_RANGE;
        else if (total_out > 0) {
            H(hipMalloc((void **)&d_out, sizeof(double2) * (size_t)total_out));
            H(hipMemcpy(d_ooff, ooff.data(), sizeof(int32_t) * ((size_t)n_polys + 1), hipMemcpyHostToDevice));
            if (rc == MESHENV_OK) {
                hipLaunchKernelGGL(k_density_rings<true>, dim3(n_polys), dim3(64), 0, nullptr, n_polys, (const int32_t *)d_off, (const double *)d_px,
                                   (const double *)d_dens, (const double2 *)d_dir, (const double *)d_len, base_length, (const int32_t *)d_ooff,
                                   d_out, d_cnt, d_st);
                H(hipGetLastError());
                H(hipDeviceSynchronize());
                H(hipMemcpy(xy_host, d_out, sizeof(double2) * (size_t)total_out, hipMemcpyDeviceToHost));
            }
        }
    }
    for (void *p : {(void *)d_off, (void *)d_px, (void *)d_cnt, (void *)d_ooff, (void *)d_dens, (void *)d_dir, (void *)d_len, (void *)d_out, (void *)d_st})
        if (p) (void)hipFree(p);
    return rc;
}

int meshenv_get_domain(MeshEnv *h, int domain, double *xy_host, int cap_points, int32_t *n_out, double *consts_host)
{
    if (!h || !n_out) return MESHENV_E_ARG;
    if (domain < 0 || domain >= h->n_domains) {
        h->err = "meshenv_get_domain: domain out of range";
        return MESHENV_E_RANGE;
    }
    MESHENV_ON_DEVICE(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const int off = h->dom_off_host[(size_t)domain], n = h->dom_off_host[(size_t)domain + 1] - off;
    *n_out = n;
    if (xy_host) {
        const int m = n < cap_points ? n : cap_points;
        HIP_TRY(h, hipMemcpy(xy_host, h->cold.dom_xy + off, sizeof(double2) * (size_t)m, hipMemcpyDeviceToHost));
    }
    if (consts_host) {
        DomConst dc;
        HIP_TRY(h, hipMemcpy(&dc, h->S.dom + domain, sizeof(dc), hipMemcpyDeviceToHost));
        consts_host[0] = dc.orig_area;
        consts_host[1] = dc.min_area;    // estimated_area_range[0] ** 2
        consts_host[2] = dc.crit_area;   // estimated_area_range[1] ** 2
    }
    return MESHENV_OK;
}

int meshenv_set_stream(MeshEnv *h, void *stream)
{
    if (!h) return MESHENV_E_ARG;
    MESHENV_ON_DEVICE(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->stream = (hipStream_t)stream;
    return MESHENV_OK;
}

int meshenv_set_packed_output(MeshEnv *h, float *msg_dev)
{
    if (!h) return MESHENV_E_ARG;
    h->S.msg = msg_dev;
    return MESHENV_OK;
}

int meshenv_num_envs(const MeshEnv *h) { return h ? h->n_envs : MESHENV_E_ARG; }
int meshenv_max_ring(const MeshEnv *h) { return h ? h->max_ring : MESHENV_E_ARG; }
int meshenv_group_size(const MeshEnv *h) { return h ? h->group : MESHENV_E_ARG; }
static const StepVariantRow &step_row(const MeshEnv *h, bool multi) { return kStepVariants[select_step_variant(step_facts(h, multi))]; }
int meshenv_step_kernel(const MeshEnv *h) { return h ? step_row(h, false).code : MESHENV_E_ARG; }
int meshenv_rollout_kernel(const MeshEnv *h) { return h ? step_row(h, true).code : MESHENV_E_ARG; }
const char *meshenv_step_kernel_name(const MeshEnv *h) { return h ? step_row(h, false).name : nullptr; }
const char *meshenv_rollout_kernel_name(const MeshEnv *h) { return h ? step_row(h, true).name : nullptr; }
int meshenv_libm_exact(const MeshEnv *h) { return h ? h->libm_exact : MESHENV_E_ARG; }
int meshenv_atan2_exact(void) { return atan_host().mode == 2 ? 1 : 0; }

int meshenv_reset_static(MeshEnv *h, const uint8_t *mask_dev, float *obs_dev, int is_static)
{
    if (!h) return MESHENV_E_ARG;
    MESHENV_ON_DEVICE(h);
    hipLaunchKernelGGL(k_reset, dim3(h->n_envs), dim3(64), h->lds, h->stream, h->S, h->cap, mask_dev, obs_dev, 0,
                       (unsigned long long)h->steps_done, is_static ? 1 : 0, h->nv_count, h->nv_meta);
    HIP_TRY(h, hipGetLastError());
    if (!mask_dev) h->front_moved = false;   // every ring is its domain's again: multiples of 1e-4 only
    return MESHENV_OK;
}

int meshenv_reset(MeshEnv *h, const uint8_t *mask_dev, float *obs_dev) { return meshenv_reset_static(h, mask_dev, obs_dev, 0); }

// The front smoother's tan / cos values (csrc/meshenv_smooth.h, "kFt..."): every argument derives from a clockwise angle
// quantised to 1e-4 rad or from a literal, so the host evaluates them all once with ITS libm -- the one the reference's
// math.tan / math.cos call -- in exactly the reference's expression order (math.radians(x) = x * (pi / 180),
// math.degrees(x) = x * (180 / pi); general/mesh.py:809, 839, 872, 886, 953-972, 1048).
static void fill_front_tables(std::vector<double> &t)
{
    // volatile: the calls below must reach the libm of the running process, not be folded by the compiler
    volatile double pi_v = 3.141592653589793;
    const double pi = pi_v, to_rad = pi / 180.0, to_deg = 180.0 / pi;
    t.assign(kFtTotal, 0.0);
    for (int q = 0; q < kFtQ; q++) {
        const double v_angle = ((double)q / 1e4) * to_deg;
        t[kFtCosInd + q] = std::cos(((360 - v_angle) / 2) * to_rad);
    }
    t[kFtTan45] = std::tan(45.0 * to_rad);
    for (int k = 0; k < 10; k++) t[kFtCosSide + k] = std::cos((45.0 - 5.0 * k) * to_rad);
    for (int row = 0; row <= kFtMidQ1 - kFtMidQ0 + 1; row++) {
        double target = row == 0 ? 45.0 : ((double)(kFtMidQ0 + row - 1) / 1e4) * to_deg;
        for (int k = 0; k < kFtMidSteps; k++) {
            t[kFtTanMid + row * kFtMidSteps + k] = std::tan((target / 2) * to_rad);
            target += 5;
        }
    }
    // get_radius_points' bisector (general/components.py:1227-1237): math.cos / math.sin of theta / 2 and of the rotation angle
    for (int q = 0; q < kFtQ; q++) {
        const double a = (double)q / 1e4;
        t[kFtSinCosFull + 2 * q] = std::sin(a);
        t[kFtSinCosFull + 2 * q + 1] = std::cos(a);
        t[kFtSinCosHalf + 2 * q] = std::sin(a / 2);
        t[kFtSinCosHalf + 2 * q + 1] = std::cos(a / 2);
    }
}

// csrc/meshenv_libm.h against the libm of this process: 2^18 arguments m * 2^e, m in [1, 2), e in [-40, 24], both signs
// (the range of coordinate differences and of the quadratic formulas' terms), plus the exact powers of two.
static int validate_pow2()
{
    volatile double two = 2.0;   // keeps the compiler from turning pow(x, 2) into x * x
    unsigned long long s = 88172645463325252ULL;
    for (int n = 0; n < (1 << 18); n++) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        const double m = 1.0 + (double)(s >> 12) / 4503599627370496.0;
        double x = std::ldexp(n < 128 ? 1.0 : m, (int)((s >> 3) % 65) - 40);
        if (s & 1) x = -x;
        if (std::pow(x, two) != pow2_glibc(x)) return 0;
    }
    return 1;
}

// the host-libm table and the pow2 validation, on first use (the smoothing entry points and meshenv_move)
static int ensure_libm_tables(MeshEnv *h)
{
    if (h->front_tab) return MESHENV_OK;
    MESHENV_ON_DEVICE(h);
    if (h->libm_exact < 0) {
        const char *off = std::getenv("MESHENV_LIBM_EXACT");   // "0": square exactly (x * x) whatever the libm does
        h->libm_exact = (off && off[0] == '0') ? 0 : validate_pow2();
    }
    double *tab_dev = nullptr;
    const int rc = dev_alloc(h, &tab_dev, (size_t)kFtTotal);
    if (rc != MESHENV_OK) return rc;
    std::vector<double> tab;
    fill_front_tables(tab);
    // synchronous copy from pageable memory: the vector goes out of scope right after
    HIP_TRY(h, hipMemcpy(tab_dev, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    h->front_tab = tab_dev;   // only now: a failed copy leaves "no table" and the next call tries again
    return MESHENV_OK;
}

// buffers and kernel attributes of the smoothing entry points, on first use
static int ensure_smooth_state(MeshEnv *h)
{
    if (h->smooth_ready) return MESHENV_OK;
    MESHENV_ON_DEVICE(h);
    int rc = ensure_libm_tables(h);
    if (rc != MESHENV_OK) return rc;
    if (!h->smooth_sweeps) rc = dev_alloc(h, &h->smooth_sweeps, (size_t)h->n_envs);
    if (rc != MESHENV_OK) return rc;
    if (!h->front_code) rc = dev_alloc(h, &h->front_code, (size_t)h->n_envs);
    if (rc != MESHENV_OK) return rc;
    HIP_TRY(h, hipFuncSetAttribute((const void *)k_smooth_interior, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIP_TRY(h, hipFuncSetAttribute((const void *)k_smooth_front, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIP_TRY(h, hipFuncSetAttribute((const void *)k_rebuild_candidates<0>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIP_TRY(h, hipFuncSetAttribute((const void *)k_rebuild_candidates<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIP_TRY(h, hipFuncSetAttribute((const void *)k_rebuild_candidates<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (!h->pend) rc = dev_alloc(h, &h->pend, (size_t)h->n_envs);
    if (rc != MESHENV_OK) return rc;
    if (!h->pend_obs) rc = dev_alloc(h, &h->pend_obs, (size_t)h->n_envs * kObsDim);
    if (rc != MESHENV_OK) return rc;
    HIP_TRY(h, hipMemsetAsync(h->pend, 0xff, sizeof(Reselect) * (size_t)h->n_envs, h->stream));   // n_elem = -1: nothing parked
    h->smooth_ready = true;   // only now: a failure above leaves the state "not ready" and the next call tries again
    return MESHENV_OK;
}

static LibmRef libm_ref(const MeshEnv *h)
{
    LibmRef lr;
    lr.tab = h->front_tab;   // nullptr until ensure_smooth_state ran: find_next_state then evaluates with ocml
    lr.exact = h->libm_exact > 0 ? 1 : 0;
    return lr;
}

// smooth_pave(interior=False) + find_next_state(static = is_static) for the envs of `mask_dev`; sw: [E] outcome
static int launch_full_smoothing(MeshEnv *h, const uint8_t *mask_dev, int iteration, int is_static, int32_t *sw, double *diff_dev,
                                 float *obs_dev)
{
    MESHENV_ON_DEVICE(h);
    const int log_cap = h->S.prm.log_cap;
    const dim3 grid(h->n_envs), block(64);
    h->front_moved = true;   // until the next full reset (launch_step)
    hipLaunchKernelGGL(k_smooth_front, grid, block, smooth_front_lds_bytes(h->cap, log_cap), h->stream, h->S, h->cap, mask_dev,
                       h->front_code, (const double *)h->front_tab, h->libm_exact, h->move_ready ? h->nv_xy : nullptr,
                       (const int32_t *)h->nv_count, (const int32_t *)h->nv_gid);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(k_smooth_interior, grid, block, smooth_lds_bytes(h->cap, log_cap), h->stream, h->S, h->cap, 0, mask_dev,
                       h->front_code, iteration, sw, diff_dev);
    HIP_TRY(h, hipGetLastError());
    if (is_static)
        hipLaunchKernelGGL(k_rebuild_candidates<2>, grid, block, h->lds, h->stream, h->S, h->cap, mask_dev, sw, h->pend, h->pend_obs,
                           obs_dev, libm_ref(h));
    else
        hipLaunchKernelGGL(k_rebuild_candidates<1>, grid, block, h->lds, h->stream, h->S, h->cap, mask_dev, sw, h->pend, h->pend_obs,
                           obs_dev, libm_ref(h));
    HIP_TRY(h, hipGetLastError());
    return MESHENV_OK;
}

static bool smoothing_fits(const MeshEnv *h, bool with_front)
{
    const int log_cap = h->S.prm.log_cap;
    if (log_cap <= 0 || h->cap + log_cap > 65535) return false;
    if (smooth_lds_bytes(h->cap, log_cap) > 160 * 1024) return false;
    return !with_front || smooth_front_lds_bytes(h->cap, log_cap) <= 160 * 1024;
}

static int ensure_move_state(MeshEnv *h)
{
    if (h->move_ready) return MESHENV_OK;
    const size_t total = (size_t)h->n_envs * (size_t)h->cap;
    int rc = MESHENV_OK;
    if (!h->nv_xy) rc = dev_alloc(h, &h->nv_xy, total);
    if (rc != MESHENV_OK) return rc;
    if (!h->nv_count) rc = dev_alloc(h, &h->nv_count, (size_t)h->n_envs);
    if (rc != MESHENV_OK) return rc;
    HIP_TRY(h, hipMemsetAsync(h->nv_count, 0, sizeof(int32_t) * (size_t)h->n_envs, h->stream));
    if (!h->nv_gid) rc = dev_alloc(h, &h->nv_gid, total);
    if (rc != MESHENV_OK) return rc;
    if (!h->nv_meta) rc = dev_alloc(h, &h->nv_meta, (size_t)h->n_envs * kNvMeta);
    if (rc != MESHENV_OK) return rc;
    HIP_TRY(h, hipMemsetAsync(h->nv_meta, 0, sizeof(int32_t) * (size_t)h->n_envs * kNvMeta, h->stream));
    if (!h->move_mask) rc = dev_alloc(h, &h->move_mask, (size_t)h->n_envs);
    if (rc != MESHENV_OK) return rc;
    if (move_lds_bytes(h->cap) > 64 * 1024)
    {
        HIP_TRY(h, hipFuncSetAttribute((const void *)k_move, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        HIP_TRY(h, hipFuncSetAttribute((const void *)k_move_skip, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    }
    h->move_ready = true;   // only now (see ensure_smooth_state)
    return MESHENV_OK;
}

// meshenv_move; skip_dev (meshenv_move_fnn_multi: the finished envs) is left out of k_move and, by its code, of the smoothing
static int move_impl(MeshEnv *h, const double *points_dev, const double *type_dev, float *obs_dev, uint8_t *done_dev,
                     uint8_t *complete_dev, uint8_t *code_dev, const uint8_t *skip_dev)
{
    if (!h) return MESHENV_E_ARG;
    if (!points_dev || !type_dev || !obs_dev || !done_dev || !complete_dev || !code_dev) return fail_arg(h, "meshenv_move: null device pointer");
    if (move_lds_bytes(h->cap) > 160 * 1024) return fail_arg(h, "meshenv_move: ring too long for the move kernel's LDS (60 B per vertex)");
    MESHENV_ON_DEVICE(h);
    int rc = ensure_move_state(h);
    if (rc == MESHENV_OK) rc = ensure_libm_tables(h);   // before the first k_move: every move computes its observation alike
    if (rc != MESHENV_OK) return rc;
    if (!skip_dev)
        hipLaunchKernelGGL(k_move, dim3(h->n_envs), dim3(64), move_lds_bytes(h->cap), h->stream, h->S, h->cap, points_dev, type_dev,
                           obs_dev, done_dev, complete_dev, code_dev, h->nv_xy, h->nv_count, h->nv_gid, libm_ref(h));
    else
        hipLaunchKernelGGL(k_move_skip, dim3(h->n_envs), dim3(64), move_lds_bytes(h->cap), h->stream, h->S, h->cap, points_dev,
                           type_dev, obs_dev, done_dev, complete_dev, code_dev, h->nv_xy, h->nv_count, h->nv_gid, libm_ref(h),
                           skip_dev);
    HIP_TRY(h, hipGetLastError());
    if (smoothing_fits(h, true)) {
        // B:405-426: the envs k_move left at "no selectable reference vertex" go through smooth_pave and select again
        const int rcs = ensure_smooth_state(h);
        if (rcs != MESHENV_OK) return rcs;
        const int nb = (h->n_envs + 255) / 256;
        hipLaunchKernelGGL(k_move_mask, dim3(nb), dim3(256), 0, h->stream, code_dev, h->move_mask, h->n_envs);
        HIP_TRY(h, hipGetLastError());
        const int rcf = launch_full_smoothing(h, h->move_mask, 400, 1, h->smooth_sweeps, nullptr, obs_dev);
        if (rcf != MESHENV_OK) return rcf;
        hipLaunchKernelGGL(k_move_finish, dim3(nb), dim3(256), 0, h->stream, h->S, h->cap, h->move_mask, h->smooth_sweeps, h->nv_count,
                           h->nv_gid, h->nv_meta, done_dev, complete_dev, code_dev);
        HIP_TRY(h, hipGetLastError());
    }
    if (h->reselect_pending) {  // move() ends with its own selection from the list, accepted or not: nothing stays parked
        HIP_TRY(h, hipMemsetAsync(h->pend, 0xff, sizeof(Reselect) * (size_t)h->n_envs, h->stream));
        h->reselect_pending = false;
    }
    return MESHENV_OK;
}

int meshenv_move(MeshEnv *h, const double *points_dev, const double *type_dev, float *obs_dev, uint8_t *done_dev,
                 uint8_t *complete_dev, uint8_t *code_dev)
{
    return move_impl(h, points_dev, type_dev, obs_dev, done_dev, complete_dev, code_dev, nullptr);
}

int meshenv_smooth(MeshEnv *h, int which, const uint8_t *mask_dev, int iteration, int interior, int is_static, int32_t *sweeps_dev,
                   double *diff_dev, float *obs_dev)
{
    if (!h || (which != 0 && which != 1)) return MESHENV_E_ARG;
    if (iteration < 0) return fail_arg(h, "meshenv_smooth: iteration must be >= 0");
    if (which && !interior)
        return fail_arg(h, "meshenv_smooth: the archived episode (which = 1) has no front to step on: interior must be != 0");
    const int log_cap = h->S.prm.log_cap;
    if (log_cap <= 0) {
        h->err = "meshenv_smooth: handle was created with log_capacity = 0 (the mesh graph is rebuilt from the element log)";
        return MESHENV_E_STATE;
    }
    const size_t lds = smooth_lds_bytes(h->cap, log_cap), lds_front = smooth_front_lds_bytes(h->cap, log_cap);
    if (lds > 160 * 1024 || (!interior && lds_front > 160 * 1024) || h->cap + log_cap > 65535)
        return fail_arg(h, "meshenv_smooth: ring stride + log_capacity too large for the smoother's LDS (16 B per ring slot + 60 B per logged vertex; front smoother 51 B per vertex)");
    MESHENV_ON_DEVICE(h);
    {
        const int rc = ensure_smooth_state(h);
        if (rc != MESHENV_OK) return rc;
    }
    int32_t *sw = sweeps_dev ? sweeps_dev : h->smooth_sweeps;
    if (!interior) return launch_full_smoothing(h, mask_dev, iteration, is_static, sw, diff_dev, obs_dev);
    const dim3 grid(h->n_envs), block(64);
    hipLaunchKernelGGL(k_smooth_interior, grid, block, lds, h->stream, h->S, h->cap, which, mask_dev, (const int32_t *)nullptr,
                       iteration, sw, diff_dev);
    HIP_TRY(h, hipGetLastError());
    if (which) return MESHENV_OK;   // an archived mesh: nothing to step on, no candidate list
    hipLaunchKernelGGL(k_rebuild_candidates<0>, grid, block, h->lds, h->stream, h->S, h->cap, mask_dev, sw, h->pend, h->pend_obs,
                       (float *)nullptr, libm_ref(h));
    HIP_TRY(h, hipGetLastError());
    h->reselect_pending = true;
    return MESHENV_OK;
}

int meshenv_smooth_final(MeshEnv *h, int which, const uint8_t *mask_dev, int iteration, double lr_1, double lr_2,
                         int32_t *sweeps_dev, double *diff_dev)
{
    if (!h || (which != 0 && which != 1)) return MESHENV_E_ARG;
    if (iteration < 0) return fail_arg(h, "meshenv_smooth_final: iteration must be >= 0");
    const int log_cap = h->S.prm.log_cap;
    if (log_cap <= 0) {
        h->err = "meshenv_smooth_final: handle was created with log_capacity = 0 (the mesh graph is rebuilt from the element log)";
        return MESHENV_E_STATE;
    }
    const size_t lds = smooth_final_lds_bytes(h->cap, log_cap);
    if (lds > 160 * 1024 || h->cap + log_cap > 65535)
        return fail_arg(h, "meshenv_smooth_final: ring stride + log_capacity too large for the smoother's LDS (51 B per vertex)");
    MESHENV_ON_DEVICE(h);
    if (!h->smooth_final_ready) {
        HIP_TRY(h, hipFuncSetAttribute((const void *)k_smooth_final, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        h->smooth_final_ready = true;
    }
    hipLaunchKernelGGL(k_smooth_final, dim3(h->n_envs), dim3(64), lds, h->stream, h->S, h->cap, which, mask_dev, iteration, lr_1,
                       lr_2, sweeps_dev, diff_dev);
    HIP_TRY(h, hipGetLastError());
    return MESHENV_OK;
}

int meshenv_get_not_valid(MeshEnv *h, int env, double *xy_host, int cap_points, int32_t *count)
{
    if (!h || !count) return MESHENV_E_ARG;
    if (env < 0 || env >= h->n_envs) {
        h->err = "meshenv_get_not_valid: env out of range";
        return MESHENV_E_RANGE;
    }
    *count = 0;
    if (!h->move_ready) return MESHENV_OK;  // move() never called: the list is empty
    MESHENV_ON_DEVICE(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    int32_t n = 0;
    HIP_TRY(h, hipMemcpy(&n, h->nv_count + env, sizeof(n), hipMemcpyDeviceToHost));
    *count = n;
    if (xy_host && n > 0) {
        const int m = n < cap_points ? n : cap_points;
        HIP_TRY(h, hipMemcpy(xy_host, h->nv_xy + (size_t)env * h->cap, sizeof(double2) * (size_t)m, hipMemcpyDeviceToHost));
    }
    return MESHENV_OK;
}

int meshenv_get_not_valid_ids(MeshEnv *h, int env, int32_t *ids_host, int cap_ids, int32_t *count, int32_t *last_host)
{
    if (!h || !count) return MESHENV_E_ARG;
    if (env < 0 || env >= h->n_envs) {
        h->err = "meshenv_get_not_valid_ids: env out of range";
        return MESHENV_E_RANGE;
    }
    *count = 0;
    if (last_host) last_host[0] = last_host[1] = last_host[2] = last_host[3] = 0;
    if (!h->move_ready) return MESHENV_OK;  // move() never called
    MESHENV_ON_DEVICE(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    int32_t n = 0, meta[kNvMeta];
    HIP_TRY(h, hipMemcpy(&n, h->nv_count + env, sizeof(n), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(meta, h->nv_meta + (size_t)env * kNvMeta, sizeof(meta), hipMemcpyDeviceToHost));
    EnvScalars s;
    HIP_TRY(h, hipMemcpy(&s, h->S.scal + env, sizeof(s), hipMemcpyDeviceToHost));
    const int n0 = h->dom_off_host[s.dom + 1] - h->dom_off_host[s.dom];
    auto gid = [n0](int32_t g) { return (g & kNewBit) ? n0 + (g & ~kNewBit) : g; };
    *count = n;
    if (ids_host && n > 0) {
        const int m = n < cap_ids ? n : cap_ids;
        HIP_TRY(h, hipMemcpy(ids_host, h->nv_gid + (size_t)env * h->cap, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost));
        for (int i = 0; i < m; i++) ids_host[i] = gid(ids_host[i]);
    }
    if (last_host) {
        last_host[0] = gid(meta[1]); last_host[1] = gid(meta[2]); last_host[2] = meta[3];
        last_host[3] = meta[4] == meta[0] ? 1 : 0;
    }
    return MESHENV_OK;
}

static int launch_step(MeshEnv *h, int n_steps, const float *actions_dev, float *obs_dev, double *reward_dev,
                       uint8_t *done_dev, uint8_t *complete_dev, float *terminal_obs_dev, int auto_reset)
{
    if (!h) return MESHENV_E_ARG;
    if (!actions_dev || !obs_dev || !reward_dev || !done_dev || !complete_dev) return fail_arg(h, "meshenv_step: null device pointer");
    if (n_steps <= 0) return fail_arg(h, "meshenv_rollout: n_steps must be positive");
    if (n_steps > 1 && h->reselect_pending) {
        h->err = "meshenv_rollout: the first step after meshenv_smooth must be a meshenv_step (it commits the re-selection "
                 "the candidate rebuild parked, include/meshenv.h)";
        return MESHENV_E_STATE;
    }
    MESHENV_ON_DEVICE(h);
    const size_t slot = (size_t)(h->ev_count % MESHENV_TIMING_POOL);
    const long long pos = h->timing > 0 ? (h->launch_count++ % (2LL * h->timing)) : -1;
    if (pos == 0) HIP_TRY(h, hipEventRecord(h->ev[2 * slot], h->stream));
    const StepVariant v = select_step_variant(step_facts(h, n_steps > 1));
    if (v < kStepGroupVariants) {
        const int G = h->group;
        GroupArgs A;
        A.S = h->S;
        A.outs.obs_out = obs_dev; A.outs.reward = reward_dev; A.outs.done = done_dev; A.outs.complete = complete_dev;
        A.outs.term_obs = terminal_obs_dev;
        A.actions = actions_dev;
        A.step0 = (unsigned long long)h->steps_done;
        A.cap = h->cap;
        A.auto_reset = auto_reset;
        A.env_lds = h->env_lds;
        A.ho_off = h->ho_off;
        A.pad = 0;
        hipLaunchKernelGGL(kGroupKernels[v], dim3((h->n_envs + G - 1) / G), dim3(64 * G), h->group_lds, h->stream, MESHENV_ENTRY_LAUNCH(A) A);
    } else {
        // bit 1: record-first staging, bit 2: key-less staging -- throughput regime only, decided in meshenv_create
        if (n_steps == 1) auto_reset = (auto_reset ? 1 : 0) | h->stage_bits;
        KStepArgs ka;
        ka.S = h->S; ka.cap = h->cap; ka.n_steps = n_steps; ka.actions = actions_dev; ka.obs_out = obs_dev;
        ka.reward = reward_dev; ka.done = done_dev; ka.complete = complete_dev; ka.term_obs = terminal_obs_dev;
        ka.auto_reset = auto_reset; ka.step0 = (unsigned long long)h->steps_done;
        hipLaunchKernelGGL(kWaveKernels[v - kStepGroupVariants], dim3(h->n_envs), dim3(64), h->lds, h->stream, ka);
    }
    HIP_TRY(h, hipGetLastError());
    if (h->reselect_pending) {  // the step after a candidate rebuild: envs whose action was rejected take the parked selection
        hipLaunchKernelGGL(k_apply_reselect, dim3(h->n_envs), dim3(64), 0, h->stream, h->S, h->pend, h->pend_obs, obs_dev);
        HIP_TRY(h, hipGetLastError());
        h->reselect_pending = false;
    }
    h->steps_done += (uint64_t)n_steps;
    if (pos >= 0 && pos == h->timing - 1) {
        HIP_TRY(h, hipEventRecord(h->ev[2 * slot + 1], h->stream));
        h->ev_count += 1;
    }
    return MESHENV_OK;
}

int meshenv_step(MeshEnv *h, const float *actions_dev, float *obs_dev, double *reward_dev, uint8_t *done_dev,
                 uint8_t *complete_dev, float *terminal_obs_dev, int auto_reset)
{
    return launch_step(h, 1, actions_dev, obs_dev, reward_dev, done_dev, complete_dev, terminal_obs_dev, auto_reset);
}

int meshenv_rollout(MeshEnv *h, int n_steps, const float *actions_dev, float *obs_dev, double *reward_dev,
                    uint8_t *done_dev, uint8_t *complete_dev, int auto_reset)
{
    return launch_step(h, n_steps, actions_dev, obs_dev, reward_dev, done_dev, complete_dev, nullptr, auto_reset);
}

__global__ void k_status(DevState S, uint8_t *out)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < S.n_envs) out[e] = (uint8_t)(S.scal[e].status & 3);  // public MESHENV_ST_* bits only
}

int meshenv_get_status(MeshEnv *h, uint8_t *status_dev)
{
    if (!h || !status_dev) return MESHENV_E_ARG;
    MESHENV_ON_DEVICE(h);
    hipLaunchKernelGGL(k_status, dim3((h->n_envs + 255) / 256), dim3(256), 0, h->stream, h->S, status_dev);
    HIP_TRY(h, hipGetLastError());
    return MESHENV_OK;
}

int meshenv_get_state(MeshEnv *h, int env, int32_t *ring_ids_host, double *ring_xy_host, double *cand_key_host,
                      int32_t *cand_stamp_host, int32_t *scalars_host, double *fscalars_host)
{
    if (!h) return MESHENV_E_ARG;
    if (env < 0 || env >= h->n_envs) {
        h->err = "meshenv_get_state: env out of range";
        return MESHENV_E_RANGE;
    }
    MESHENV_ON_DEVICE(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    EnvScalars s;
    HIP_TRY(h, hipMemcpy(&s, h->S.scal + env, sizeof(s), hipMemcpyDeviceToHost));
    const size_t off = (size_t)env * (size_t)h->cap;
    const int n0 = h->dom_off_host[s.dom + 1] - h->dom_off_host[s.dom];
    const int n = s.n;
    if (ring_ids_host) {
        HIP_TRY(h, hipMemcpy(ring_ids_host, h->S.ring_id + off, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++)  // k-th new vertex -> global id n0 + k (index in boundary.vertices)
            if (ring_ids_host[i] & kNewBit) ring_ids_host[i] = n0 + (ring_ids_host[i] & ~kNewBit);
    }
    if (ring_xy_host) HIP_TRY(h, hipMemcpy(ring_xy_host, h->S.ring_xy + off, sizeof(double2) * n, hipMemcpyDeviceToHost));
    if (cand_stamp_host || cand_key_host) {
        std::vector<int32_t> st((size_t)n);
        std::vector<double> ky((size_t)n);
        HIP_TRY(h, hipMemcpy(st.data(), h->S.ring_stamp + off, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(ky.data(), h->S.ring_key + off, sizeof(double) * n, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) {
            if (cand_stamp_host) cand_stamp_host[i] = st[i];
            if (cand_key_host) cand_key_host[i] = st[i] == kNotCand ? NAN : ky[i];
        }
    }
    if (scalars_host) {
        scalars_host[0] = s.n;
        scalars_host[1] = s.ref;
        scalars_host[2] = s.n_elem;
        scalars_host[3] = s.failed;
        scalars_host[4] = n0 + s.n_new;
        scalars_host[5] = s.status & 3;
        scalars_host[6] = s.dom;
        scalars_host[7] = n0;
    }
    if (fscalars_host) {
        fscalars_host[0] = s.area;
        fscalars_host[1] = s.bl;
    }
    return MESHENV_OK;
}

// shared body of meshenv_get_elements (which = 0) and meshenv_get_last_episode (which = 1)
static int fetch_elements(MeshEnv *h, const char *fn, int which, int env, int32_t *quads_host, int cap_elems,
                          double *vertex_xy_host, int cap_verts, int32_t *n_elem, int32_t *n_vert, int32_t *flags,
                          int32_t *episodes)
{
    if (!h || !n_elem || !n_vert) return MESHENV_E_ARG;
    if (env < 0 || env >= h->n_envs) {
        h->err = std::string(fn) + ": env out of range";
        return MESHENV_E_RANGE;
    }
    const int cap = h->S.prm.log_cap;
    if (cap <= 0) {
        h->err = std::string(fn) + ": handle was created with log_capacity = 0";
        return MESHENV_E_STATE;
    }
    MESHENV_ON_DEVICE(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    EnvScalars s;
    HIP_TRY(h, hipMemcpy(&s, h->S.scal + env, sizeof(s), hipMemcpyDeviceToHost));
    int half = (s.status >> 4) & 1, ne = s.n_elem, nnew = s.n_new;
    if (which) {
        LastEpisode le;
        HIP_TRY(h, hipMemcpy(&le, h->cold.last_ep + env, sizeof(le), hipMemcpyDeviceToHost));
        half ^= 1; ne = le.n_elem; nnew = le.n_new;
        if (flags) *flags = le.flags;
        if (episodes) *episodes = le.episodes;
    }
    const int d = s.dom;
    const int n0 = h->dom_off_host[d + 1] - h->dom_off_host[d];
    ne = ne < cap ? ne : cap;
    nnew = nnew < cap ? nnew : cap;
    if (ne > cap_elems) ne = cap_elems;
    int nv = n0 + nnew;
    if (nv > cap_verts) nv = cap_verts;
    const size_t base = ((size_t)env * 2 + half) * cap;
    if (quads_host && ne > 0) {
        HIP_TRY(h, hipMemcpy(quads_host, h->cold.log_quads + base * 4, sizeof(int32_t) * 4 * (size_t)ne, hipMemcpyDeviceToHost));
        for (int i = 0; i < 4 * ne; i++)
            if (quads_host[i] & kNewBit) quads_host[i] = n0 + (quads_host[i] & ~kNewBit);
    }
    if (vertex_xy_host && nv > 0) {
        const int first = nv < n0 ? nv : n0;
        HIP_TRY(h, hipMemcpy(vertex_xy_host, h->cold.dom_xy + h->dom_off_host[d], sizeof(double2) * (size_t)first, hipMemcpyDeviceToHost));
        if (nv > n0)
            HIP_TRY(h, hipMemcpy(vertex_xy_host + 2 * (size_t)n0, h->cold.log_vxy + base, sizeof(double2) * (size_t)(nv - n0), hipMemcpyDeviceToHost));
    }
    *n_elem = ne;
    *n_vert = nv;
    return MESHENV_OK;
}

int meshenv_get_elements(MeshEnv *h, int env, int32_t *quads_host, int cap_elems, double *vertex_xy_host,
                         int cap_verts, int32_t *n_elem, int32_t *n_vert)
{
    return fetch_elements(h, "meshenv_get_elements", 0, env, quads_host, cap_elems, vertex_xy_host, cap_verts, n_elem,
                          n_vert, nullptr, nullptr);
}

int meshenv_get_last_episode(MeshEnv *h, int env, int32_t *quads_host, int cap_elems, double *vertex_xy_host,
                             int cap_verts, int32_t *n_elem, int32_t *n_vert, int32_t *flags, int32_t *episodes)
{
    return fetch_elements(h, "meshenv_get_last_episode", 1, env, quads_host, cap_elems, vertex_xy_host, cap_verts,
                          n_elem, n_vert, flags, episodes);
}

int meshenv_element_quality(MeshEnv *h, int which, double *elem_dev, double *stats_dev, int32_t *count_dev)
{
    if (!h || (which != 0 && which != 1)) return MESHENV_E_ARG;
    if (h->S.prm.log_cap <= 0) {
        h->err = "meshenv_element_quality: handle was created with log_capacity = 0";
        return MESHENV_E_STATE;
    }
    MESHENV_ON_DEVICE(h);
    hipLaunchKernelGGL(k_element_quality, dim3(h->n_envs), dim3(64), 0, h->stream, h->S, which, elem_dev, stats_dev,
                       count_dev);
    HIP_TRY(h, hipGetLastError());
    return MESHENV_OK;
}

static_assert(MESHENV_TOPOLOGY_DIM == kTopologyDim && MESHENV_TOPO_MASKED == kTopoMasked && MESHENV_TOPO_LOG_OVERFLOW == kTopoLogOverflow &&
              MESHENV_TOPO_DEGREE == kTopoDegree && MESHENV_TOPO_NOT_ARCHIVED == kTopoNotArchived,
              "include/meshenv_topology.h and csrc/meshenv_topology.h disagree");

int meshenv_mesh_topology(MeshEnv *h, int which, const uint8_t *mask_dev, int32_t *report_dev, uint8_t *valence_dev)
{
    if (!h) return MESHENV_E_ARG;
    if (which != 0 && which != 1) return fail_arg(h, "meshenv_mesh_topology: which must be 0 (running) or 1 (archived)");
    if (!report_dev) return fail_arg(h, "meshenv_mesh_topology: report_dev is NULL");
    const int log_cap = h->S.prm.log_cap;
    if (log_cap <= 0) {
        h->err = "meshenv_mesh_topology: handle was created with log_capacity = 0 (the mesh is read from the element log)";
        return MESHENV_E_STATE;
    }
    if (h->max_ring + log_cap > 65535)
        return fail_arg(h, "meshenv_mesh_topology: max ring + log_capacity must be <= 65535 (16-bit vertex indices)");
    MESHENV_ON_DEVICE(h);
    hipLaunchKernelGGL(k_mesh_topology, dim3(h->n_envs), dim3(64), 0, h->stream, h->S, which, mask_dev, report_dev, valence_dev,
                       h->max_ring + log_cap);
    HIP_TRY(h, hipGetLastError());
    return MESHENV_OK;
}

int meshenv_eval_set_topology(MeshEnv *h, int32_t *ep_topology_dev)
{
    if (!h) return MESHENV_E_ARG;
    if (ep_topology_dev && (h->S.prm.log_cap <= 0 || h->max_ring + h->S.prm.log_cap > 65535)) {
        h->err = "meshenv_eval_set_topology: needs a handle created with 0 < log_capacity <= 65535 - max ring";
        return MESHENV_E_STATE;
    }
    h->eval_topology = ep_topology_dev;
    return MESHENV_OK;
}

int meshenv_topology_selftest(int device, int n_meshes, const int32_t *elem_offsets_host, const int32_t *quads_host,
                              const int32_t *n0_host, const int32_t *n_new_host, int width, int32_t *report_host,
                              uint8_t *valence_host)
{
    if (n_meshes <= 0 || !elem_offsets_host || !quads_host || !n0_host || !n_new_host || !report_host) return MESHENV_E_ARG;
    if (width <= 0 || width > 65535 || elem_offsets_host[0] != 0) return MESHENV_E_ARG;
    for (int m = 0; m < n_meshes; m++) {
        if (elem_offsets_host[m + 1] < elem_offsets_host[m] || n0_host[m] < 3 || n_new_host[m] < 0 ||
            (long long)n0_host[m] + n_new_host[m] > width)
            return MESHENV_E_ARG;
    }
    const size_t total = (size_t)elem_offsets_host[n_meshes];
    // the log's encoding: the k-th generated vertex is kNewBit | k.  An id outside the mesh is refused here; that the four
    // ids of a record are distinct is the caller's part of the contract.
    std::vector<int32_t> log(4 * (total ? total : 1), 0);
    for (int m = 0; m < n_meshes; m++) {
        const int n0 = n0_host[m], nv = n0 + n_new_host[m];
        for (size_t i = 4 * (size_t)elem_offsets_host[m]; i < 4 * (size_t)elem_offsets_host[m + 1]; i++) {
            const int id = quads_host[i];
            if (id < 0 || id >= nv) return MESHENV_E_ARG;
            log[i] = id >= n0 ? (kNewBit | (id - n0)) : id;
        }
    }
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return MESHENV_E_HIP;
    const size_t n = (size_t)n_meshes;
    int32_t *d_off = nullptr, *d_log = nullptr, *d_n0 = nullptr, *d_new = nullptr, *d_rep = nullptr;
    uint8_t *d_val = nullptr;
    bool ok = hipMalloc(&d_off, sizeof(int32_t) * (n + 1)) == hipSuccess && hipMalloc(&d_log, sizeof(int32_t) * log.size()) == hipSuccess &&
              hipMalloc(&d_n0, sizeof(int32_t) * n) == hipSuccess && hipMalloc(&d_new, sizeof(int32_t) * n) == hipSuccess &&
              hipMalloc(&d_rep, sizeof(int32_t) * n * kTopologyDim) == hipSuccess &&
              (!valence_host || hipMalloc(&d_val, n * (size_t)width) == hipSuccess);
    ok = ok && hipMemcpy(d_off, elem_offsets_host, sizeof(int32_t) * (n + 1), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_log, log.data(), sizeof(int32_t) * log.size(), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_n0, n0_host, sizeof(int32_t) * n, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_new, n_new_host, sizeof(int32_t) * n, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_rep, report_host, sizeof(int32_t) * n * kTopologyDim, hipMemcpyHostToDevice) == hipSuccess &&
         (!valence_host || hipMemcpy(d_val, valence_host, n * (size_t)width, hipMemcpyHostToDevice) == hipSuccess);
    if (ok) {
        hipLaunchKernelGGL(k_topology_selftest, dim3(n_meshes), dim3(64), 0, nullptr, d_off, reinterpret_cast<const int4 *>(d_log),
                           d_n0, d_new, d_rep, d_val, width);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    }
    ok = ok && hipMemcpy(report_host, d_rep, sizeof(int32_t) * n * kTopologyDim, hipMemcpyDeviceToHost) == hipSuccess &&
         (!valence_host || hipMemcpy(valence_host, d_val, n * (size_t)width, hipMemcpyDeviceToHost) == hipSuccess);
    (void)hipFree(d_off); (void)hipFree(d_log); (void)hipFree(d_n0); (void)hipFree(d_new); (void)hipFree(d_rep); (void)hipFree(d_val);
    return ok ? MESHENV_OK : MESHENV_E_HIP;
}

int meshenv_quad_quality(MeshEnv *h, int n, const double *quad_xy_dev, int index, double *out_dev)
{
    if (!h || n < 0 || (n > 0 && (!quad_xy_dev || !out_dev))) return MESHENV_E_ARG;
    if (!(index == 0 || index == 1 || index == 3 || index == 4 || index == 5))
        return fail_arg(h, "meshenv_quad_quality: index must be 0, 1, 3, 4 or 5 (2 and 6 add the boundary term of the extraction "
                           "step: that value is the step's reward)");
    if (n == 0) return MESHENV_OK;
    MESHENV_ON_DEVICE(h);
    hipLaunchKernelGGL(k_quad_quality, dim3((n + 63) / 64), dim3(64), 0, h->stream, n,
                       reinterpret_cast<const double2 *>(quad_xy_dev), index, out_dev);
    HIP_TRY(h, hipGetLastError());
    return MESHENV_OK;
}

int meshenv_counters(MeshEnv *h, uint64_t *out_host)
{
    if (!h || !out_host) return MESHENV_E_ARG;
    MESHENV_ON_DEVICE(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::vector<EnvCounters> c((size_t)h->n_envs);
    std::vector<EnvScalars> sc((size_t)h->n_envs);
    HIP_TRY(h, hipMemcpy(c.data(), h->S.cnt, sizeof(EnvCounters) * (size_t)h->n_envs, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(sc.data(), h->S.scal, sizeof(EnvScalars) * (size_t)h->n_envs, hipMemcpyDeviceToHost));
    uint64_t a = h->steps_done * (uint64_t)h->n_envs, b = 0, s = 0, sv = 0;
    for (int e = 0; e < h->n_envs; e++) {
        const EnvCounters &k = c[(size_t)e];
        b += k.valid;
        s += k.sum_n + (uint64_t)sc[(size_t)e].n * (h->steps_done - k.last_change);  // the running term of the lazy sum
        sv += k.sum_n_valid;
    }
    out_host[0] = a;
    out_host[1] = b;
    out_host[2] = s;
    out_host[3] = sv;
    return MESHENV_OK;
}

#ifdef MESHENV_STAMPS
// diagnostic build only: raw per-env counter records (see k_step)
int meshenv_debug_raw_counters(MeshEnv *h, uint64_t *out_host)
{
    if (!h || !out_host) return MESHENV_E_ARG;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(out_host, h->S.cnt, sizeof(EnvCounters) * (size_t)h->n_envs, hipMemcpyDeviceToHost));
    return MESHENV_OK;
}
int meshenv_debug_stamps(MeshEnv *h, uint64_t *out_host)
{
    if (!h || !out_host) return MESHENV_E_ARG;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(out_host, h->S.dbg, sizeof(uint64_t) * 16 * (size_t)h->n_envs, hipMemcpyDeviceToHost));
    return MESHENV_OK;
}
#endif

// ---- primitive self-test hook (tests/test_gpu_primitives.py): evaluates the device geometry primitives on
// caller-supplied host arrays so that they can be compared with the CPU oracle's.
__global__ void k_selftest(int what, int n, const double *in, double *out, int libm_exact)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (what == 0) out[i] = round4_py(in[i]);
    else if (what == 1) out[i] = round4_np(in[i]);
    else if (what == 2) out[i] = cw(mkp(in[6 * i], in[6 * i + 1]), mkp(in[6 * i + 2], in[6 * i + 3]), mkp(in[6 * i + 4], in[6 * i + 5]));
    else if (what == 3) out[i] = is_cross(mkp(in[8 * i], in[8 * i + 1]), mkp(in[8 * i + 2], in[8 * i + 3]), mkp(in[8 * i + 4], in[8 * i + 5]),
                                          mkp(in[8 * i + 6], in[8 * i + 7])) ? 1.0 : 0.0;
    else if (what == 4) out[i] = (sin_rounds_to_zero(in[2 * i], in[2 * i + 1]) ? 1.0 : 0.0) + (sin_rounds_to_zero_exact(in[2 * i], in[2 * i + 1]) ? 2.0 : 0.0);
    else if (what == 5) out[i] = (double)round4_npf((float)in[i]);
    else if (what == 6) out[i] = dist(mkp(in[4 * i], in[4 * i + 1]), mkp(in[4 * i + 2], in[4 * i + 3]));
    else if (what == 7) out[i] = (sqrt_pos(in[i]) == sqrt(in[i])) ? 1.0 : 0.0;  // against the compiler's IEEE sqrt
    else if (what == 8) {  // cw_fast against the exact form: 0 equal, 1 guard band raised (and equal after the fallback), 2 MISMATCH
        bool ne;
        const double f = cw_fast(in[2 * i], in[2 * i + 1], ne);
        const double e = cw_exact(in[2 * i], in[2 * i + 1]);
        out[i] = ne ? 1.0 : ((f == e && signbit(f) == signbit(e)) ? 0.0 : 2.0);
    } else if (what == 9 || what == 10) {
        // the front smoother's vertex constructions (csrc/meshenv_smooth.h): 9 doubles = which (0 middle_vertex, 1 side_vertex,
        // 2 indention_vertex), vertex, p1, p2, angle, dist; what 9 -> x, 10 -> y; NaN where the construction is undefined.
        // As in the product path the tan / cos of the angle come from the host's libm: meshenv_selftest replaces the angle
        // by math.tan(math.radians(angle / 2)) (which 0) or math.cos(math.radians(angle)) (which 1, 2) before the upload.
        const double *q = in + 9 * (size_t)i;
        FrontState f;
        f.coord = nullptr; f.adj = nullptr; f.deg = nullptr; f.ringu = nullptr; f.n = 0; f.n0 = 0; f.raised = 0; f.tab = nullptr; f.exact = libm_exact != 0;
        const P2 v = mkp(q[1], q[2]), a = mkp(q[3], q[4]), b = mkp(q[5], q[6]);
        const int which = (int)q[0];
        P2 r;
        if (which == 0) r = middle_vertex(f, v, a, b, q[7]);
        else if (which == 1) r = side_vertex(f, v, a, b, q[7], q[8], false);
        else if (which == 2) r = indention_vertex(f, v, a, b, q[7], q[8], false);
        else {  // 3: Mesh.estimate_4th_vertex(origin, left, right, factor, suggest_dist or < 0 for None)
            const double2 e = estimate_4th_vertex(make_double2(v.x, v.y), make_double2(a.x, a.y), make_double2(b.x, b.y), q[7], q[8] >= 0, q[8]);
            r = mkp(e.x, e.y);
        }
        out[i] = f.raised ? __builtin_nan("") : (what == 9 ? r.x : r.y);
    } else if (what == 11) out[i] = pow2_glibc(in[i]);   // against the host libm's pow(x, 2.0)
    else if (what == 12) out[i] = cw_exact(in[2 * i], in[2 * i + 1]);   // the quantised angle of terms (c, d)
    else if (what == 13) {   // the tie-breaker alone, against the host libm's atan2; NaN outside its domain
        bool ok;
        const double t = atan2_glibc(in[2 * i], in[2 * i + 1], g_atan_cij, ok);
        out[i] = ok ? t : __builtin_nan("");
    } else if (what == 14) out[i] = atan2_cr(in[2 * i], in[2 * i + 1]);
    else if (what == 15) out[i] = sincos_small_nc(in[i]).s;   // against the host libm's sin / cos: within an ulp
    else if (what == 16) out[i] = sincos_small_nc(in[i]).c;
    else if (what == 17) {
        // the x-slab pre-filter of the observation scan against what the unfiltered scan evaluates for one position:
        // 7 doubles = ref (x, y), p_s - ref before rounding (qx, qy), target_length, v.x, b.x -- with v = (v.x, ref.y - 1),
        // b = (b.x, ref.y + 1), an edge across the bisector's line.  out = 1 kept by the filter + 2 the bisector hits the
        // edge + 4 the fan-slot distance d(ref, v) < target_length; a position with 2 or 4 but not 1 is a dropped one.
        const double *q = in + 7 * (size_t)i;
        const P2 ref = mkp(q[0], q[1]);
        const double tl = q[4];
        const double ux = (ref.x + q[2]) - ref.x, uy = (ref.y + q[3]) - ref.y;
        const P2 v = mkp(q[5], ref.y - 1), b = mkp(q[6], ref.y + 1);
        const double W = slab_half_width(tl);
        const double slab_lo = ref.x - W, slab_hi = ref.x + W;
        double s;
        out[i] = (slab_keeps(slab_lo, slab_hi, v.x, b.x) ? 1.0 : 0.0) + (bisector_hits(ref, ux, uy, v, b, s) ? 2.0 : 0.0) +
                 (dist(ref, v) < tl ? 4.0 : 0.0);
    } else if (what == 18) {
        // the per-edge pre-filter of point_inside against is_cross: 7 doubles = p (x, y), vi (x, y), vm (x, y),
        // ray_length.  out = 1 the filter drops the edge + 2 is_cross(p -> (ray_length, p.y), vi - vm) holds; 3 = a
        // counted edge dropped.
        const double *q = in + 7 * (size_t)i;
        const P2 p = mkp(q[0], q[1]), vi = mkp(q[2], q[3]), vm = mkp(q[4], q[5]), far = mkp(q[6], q[1]);
        out[i] = (pip_filter_usable(fabs(q[6] - p.x)) && pip_edge_clear(p, vi, vm) ? 1.0 : 0.0) + (straddle(p, far, vi, vm) && straddle(vi, vm, p, far) ? 2.0 : 0.0);
    } else if (what == 19) {
        // one entry of element_quality (csrc/meshenv_quality.h) for an arbitrary quad: 9 doubles = the four vertices
        // (x, y) in Mesh.vertices order, then the record index 0-7; NaN for any other index
        const double *q = in + 9 * (size_t)i;
        P2 m[4];
        for (int k = 0; k < 4; k++) m[k] = mkp(q[2 * k], q[2 * k + 1]);
        double rec[kQualityDim];
        element_quality(m, rec);
        double r = __builtin_nan("");
        for (int k = 0; k < kQualityDim; k++) r = q[8] == (double)k ? rec[k] : r;
        out[i] = r;
    }
}

int meshenv_selftest(int device, int what, int n, int in_per_item, const double *in_host, double *out_host)
{
    if (n <= 0 || !in_host || !out_host || in_per_item <= 0) return MESHENV_E_ARG;
    if ((what == 17 || what == 18) && in_per_item != 7) return MESHENV_E_ARG;   // 7 doubles per case (k_selftest)
    if (what == 19 && in_per_item != 9) return MESHENV_E_ARG;                    // 9 doubles per case (k_selftest)
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return MESHENV_E_HIP;
    double *din = nullptr, *dout = nullptr;
    if (hipMalloc(&din, sizeof(double) * (size_t)n * in_per_item) != hipSuccess) return MESHENV_E_HIP;
    if (hipMalloc(&dout, sizeof(double) * (size_t)n) != hipSuccess) { (void)hipFree(din); return MESHENV_E_HIP; }
    int rc = MESHENV_OK;
    std::vector<double> staged;
    if ((what == 9 || what == 10) && in_per_item == 9) {   // the constructions take the host libm's tan / cos (see k_selftest)
        staged.assign(in_host, in_host + (size_t)n * 9);
        volatile double pi_v = 3.141592653589793;
        const double to_rad = pi_v / 180.0;
        for (int i = 0; i < n; i++) {
            double *q = staged.data() + 9 * (size_t)i;
            const int which = (int)q[0];
            if (which == 0) q[7] = std::tan((q[7] / 2) * to_rad);
            else if (which == 1 || which == 2) q[7] = std::cos(q[7] * to_rad);
        }
        in_host = staged.data();
    }
    if (hipMemcpy(din, in_host, sizeof(double) * (size_t)n * in_per_item, hipMemcpyHostToDevice) != hipSuccess) rc = MESHENV_E_HIP;
    if (rc == MESHENV_OK && upload_atan_state() != hipSuccess) rc = MESHENV_E_HIP;
    if (rc == MESHENV_OK) {
        hipLaunchKernelGGL(k_selftest, dim3((n + 63) / 64), dim3(64), 0, nullptr, what, n, din, dout,
                           (what == 9 || what == 10) ? validate_pow2() : 0);
        if (hipDeviceSynchronize() != hipSuccess) rc = MESHENV_E_HIP;
    }
    if (rc == MESHENV_OK && hipMemcpy(out_host, dout, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) rc = MESHENV_E_HIP;
    (void)hipFree(din);
    (void)hipFree(dout);
    return rc;
}

int meshenv_set_timing(MeshEnv *h, int enable)
{
    if (!h) return MESHENV_E_ARG;
    MESHENV_ON_DEVICE(h);
    if (enable && h->ev.empty()) {
        h->ev.resize(2 * (size_t)MESHENV_TIMING_POOL, nullptr);
        for (hipEvent_t &e : h->ev) HIP_TRY(h, hipEventCreate(&e));
    }
    h->timing = enable > 0 ? enable : 0;
    h->launch_count = 0;
    h->ev_count = 0;
    return MESHENV_OK;
}

int meshenv_kernel_times(MeshEnv *h, float *ms_host, int cap, int32_t *n_out)
{
    if (!h || !ms_host || !n_out || cap < 0) return MESHENV_E_ARG;
    MESHENV_ON_DEVICE(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    long long have = h->ev_count < MESHENV_TIMING_POOL ? h->ev_count : MESHENV_TIMING_POOL;
    if (have > cap) have = cap;
    const long long first = h->ev_count - have;
    for (long long k = 0; k < have; k++) {
        const size_t slot = (size_t)((first + k) % MESHENV_TIMING_POOL);
        HIP_TRY(h, hipEventElapsedTime(ms_host + k, h->ev[2 * slot], h->ev[2 * slot + 1]));
        ms_host[k] /= (float)(h->timing > 0 ? h->timing : 1);
    }
    *n_out = (int32_t)have;
    h->ev_count = 0;
    return MESHENV_OK;
}

// ------------------------------------------------------------------------------------------ fused SAC actor
struct MeshActor : HandleBase {
    float *buf = nullptr;  // all weights, one allocation
    size_t nfloat = 0;
    ActorWeights W{};
    bool loaded = false;
    PackTable table{};     // meshenv_actor_bind: the live tensors and where meshenv_actor_refresh packs them
    int n_copies = 0;
    bool live = false;
};

// The SAC actor's buffer, in the tensor order of meshenv_actor_bind: w1 b1 w2 b2 w3 b3, then mu at column 0 and log_std at
// column kActOut of one head tile.
static PackLayout actor_layout()
{
    PackLayout L;
    L.tower(kActHid, 3, kActIn, kActInPad / 16, kActOut, true);
    return L;
}

int meshenv_actor_create(int device, void *stream, MeshActor **out)
{
    const int rc = create_handle("meshenv_actor_create", device, stream, out);
    if (rc != MESHENV_OK) return rc;
    MeshActor *a = *out;
    a->nfloat = actor_layout().floats;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess || hipMalloc((void **)&a->buf, a->nfloat * sizeof(float)) != hipSuccess) {
        g_create_error = "meshenv_actor_create: hipMalloc failed";
        delete a;
        *out = nullptr;
        return MESHENV_E_HIP;
    }
    return MESHENV_OK;
}

void meshenv_actor_destroy(MeshActor *a) { destroy_handle(a, a ? a->buf : nullptr); }

int meshenv_actor_set_stream(MeshActor *a, void *stream) { return set_stream(a, stream); }

// weights in torch.nn.Linear layout ([out][in], row-major), host pointers
int meshenv_actor_load(MeshActor *a, const float *w1, const float *b1, const float *w2, const float *b2, const float *w3,
                       const float *b3, const float *w_mu, const float *b_mu, const float *w_log_std,
                       const float *b_log_std, const float *low, const float *high)
{
    if (!a || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !w_mu || !b_mu || !w_log_std || !b_log_std || !low || !high)
        return MESHENV_E_ARG;
    const PackLayout L = actor_layout();
    const float *const src[10] = {w1, b1, w2, b2, w3, b3, w_mu, b_mu, w_log_std, b_log_std};
    std::vector<float> h(L.floats, 0.0f);
    pack_host(L, src, h.data());
    if (h.size() > a->nfloat) {
        a->err = "meshenv_actor_load: internal size mismatch";
        return MESHENV_E_STATE;
    }
    DeviceGuard guard(a->device);
    if (guard.err != hipSuccess ||
        hipMemcpy(a->buf, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        a->err = "meshenv_actor_load: upload failed";
        return MESHENV_E_HIP;
    }
    point(a->buf, L.s, {&a->W.w1p, &a->W.b1, &a->W.w2p, &a->W.b2, &a->W.w3p, &a->W.b3, &a->W.whp, &a->W.bh});
    for (int i = 0; i < 3; i++) { a->W.low[i] = low[i]; a->W.high[i] = high[i]; }
    a->loaded = true;
    return MESHENV_OK;
}

static int actor_launch(MeshActor *a, const char *fn, int n, const float *obs_dev, const float *noise_dev,
                        float *actions_dev, int sample, uint64_t seed, uint64_t counter, float *eps_out_dev)
{
    if (!a || n <= 0 || !obs_dev || !actions_dev) return MESHENV_E_ARG;
    if (!a->loaded) {
        a->err = std::string(fn) + ": no weights loaded";
        return MESHENV_E_STATE;
    }
    DeviceGuard guard(a->device);
    return launch(a, guard, fn, [&] {
        hipLaunchKernelGGL(k_actor_forward, dim3((n + kActEnvs - 1) / kActEnvs), dim3(64 * kActWaves), 0, a->stream, a->W, n, obs_dev,
                           noise_dev, actions_dev, sample, seed, counter, eps_out_dev);
    });
}

int meshenv_actor_forward(MeshActor *a, int n, const float *obs_dev, const float *noise_dev, float *actions_dev)
{
    return actor_launch(a, "meshenv_actor_forward", n, obs_dev, noise_dev, actions_dev, 0, 0, 0, nullptr);
}

int meshenv_actor_sample(MeshActor *a, int n, const float *obs_dev, uint64_t seed, uint64_t counter, float *actions_dev,
                         float *eps_out_dev)
{
    return actor_launch(a, "meshenv_actor_sample", n, obs_dev, nullptr, actions_dev, 1, seed, counter, eps_out_dev);
}

int meshenv_step_actor(MeshEnv *h, MeshActor *a, const float *actions_dev, float *obs_dev, double *reward_dev, uint8_t *done_dev,
                       uint8_t *complete_dev, float *terminal_obs_dev, int auto_reset, int sample, uint64_t seed, uint64_t counter,
                       float *actions_next_dev, float *eps_out_dev)
{
    if (!h || !a) return MESHENV_E_ARG;
    if (!actions_dev || !obs_dev || !reward_dev || !done_dev || !complete_dev || !actions_next_dev || actions_next_dev == actions_dev)
        return fail_arg(h, "meshenv_step_actor: null device pointer, or actions_next aliases actions");
    if (!a->loaded) {
        h->err = "meshenv_step_actor: the actor has no weights loaded";
        return MESHENV_E_STATE;
    }
    if (a->device != h->device || a->stream != h->stream) {   // the two halves are ordered by the stream alone
        h->err = "meshenv_step_actor: env and actor must be on the same device and stream (meshenv_set_stream / meshenv_actor_set_stream)";
        return MESHENV_E_STATE;
    }
    const bool fusable = h->group == 16 && h->default_params && !h->front_moved && !h->env_lds &&
                         h->timing == 0 && !h->reselect_pending && group_actor_lds_bytes(h->cap) <= 160 * 1024;
    if (!fusable) {   // same results by two launches (other batch sizes / ring lengths, timing armed, the
                      // step after meshenv_smooth whose parked re-selection changes the observation the policy reads)
        const int rc = launch_step(h, 1, actions_dev, obs_dev, reward_dev, done_dev, complete_dev, terminal_obs_dev, auto_reset);
        if (rc != MESHENV_OK) return rc;
        const int ra = actor_launch(a, "meshenv_step_actor", h->n_envs, obs_dev, nullptr, actions_next_dev, sample, seed, counter,
                                    eps_out_dev);
        if (ra != MESHENV_OK) h->err = a->err;
        return ra;
    }
    MESHENV_ON_DEVICE(h);
    if (!h->fused_ready) {
        HIP_TRY(h, hipFuncSetAttribute((const void *)k_step_group_actor<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        HIP_TRY(h, hipFuncSetAttribute((const void *)k_step_group_actor<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        h->fused_ready = true;
    }
    GroupActorArgs GA;
    GA.g.S = h->S;
    GA.g.outs.obs_out = obs_dev; GA.g.outs.reward = reward_dev; GA.g.outs.done = done_dev; GA.g.outs.complete = complete_dev;
    GA.g.outs.term_obs = terminal_obs_dev;
    GA.g.actions = actions_dev;
    GA.g.step0 = (unsigned long long)h->steps_done;
    GA.g.cap = h->cap;
    GA.g.env_lds = nullptr; GA.g.ho_off = 0; GA.g.pad = 0;
    GA.g.auto_reset = auto_reset;
    GA.W = a->W;
    GA.actions_next = actions_next_dev;
    GA.eps_out = eps_out_dev;
    GA.seed = seed; GA.counter = counter;
    GA.sample = sample ? 1 : 0; GA.pad = 0;
    if (step_small_ring(h->cap)) hipLaunchKernelGGL((k_step_group_actor<true, true>), dim3((h->n_envs + 15) / 16), dim3(64 * 16), group_actor_lds_bytes(h->cap), h->stream, MESHENV_ENTRY_LAUNCH(GA.g) GA);
    else hipLaunchKernelGGL((k_step_group_actor<true>), dim3((h->n_envs + 15) / 16), dim3(64 * 16), group_actor_lds_bytes(h->cap), h->stream, MESHENV_ENTRY_LAUNCH(GA.g) GA);
    HIP_TRY(h, hipGetLastError());
    h->steps_done += 1;
    return MESHENV_OK;
}

int meshenv_extract_samples(MeshEnv *h, int which, const uint8_t *mask_dev, int n_neighbor, int n_radius, double radius, int index,
                            double quality_threshold, int64_t *count_dev, uint8_t *status_dev, const int64_t *offsets_dev,
                            double *samples_dev, double *outputs_dev, double *types_dev)
{
    if (!h || (which != 0 && which != 1) || !count_dev || !status_dev) return MESHENV_E_ARG;
    if (n_neighbor < 1 || n_neighbor > kSampMaxNeighbor || n_radius < 1 || n_radius > kSampMaxRadius || !(radius > 0) ||
        (index != 1 && index != 5))
        return fail_arg(h, "meshenv_extract_samples: n_neighbor in 1..3, n_radius in 1..4, radius > 0 and index 1 or 5 (the values of the reference's callers) are supported");
    if (offsets_dev && (!samples_dev || !outputs_dev || !types_dev))
        return fail_arg(h, "meshenv_extract_samples: offsets_dev given without the three output arrays");
    const int log_cap = h->S.prm.log_cap;
    if (log_cap <= 0) {
        h->err = "meshenv_extract_samples: handle was created with log_capacity = 0 (the mesh graph is rebuilt from the element log)";
        return MESHENV_E_STATE;
    }
    const size_t lds = samples_lds_bytes(h->cap, log_cap);
    if (lds > 160 * 1024 || h->cap + log_cap > 65535)
        return fail_arg(h, "meshenv_extract_samples: ring stride + log_capacity too large for the kernel's LDS (49 B per vertex)");
    MESHENV_ON_DEVICE(h);
    int rc = ensure_libm_tables(h);
    if (rc != MESHENV_OK) return rc;
    if (!h->samples_ready) {
        HIP_TRY(h, hipFuncSetAttribute((const void *)k_extract_samples<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        HIP_TRY(h, hipFuncSetAttribute((const void *)k_extract_samples<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        h->samples_ready = true;
    }
    SampleParams P;
    P.n_neighbor = n_neighbor; P.n_radius = n_radius; P.index = index; P.radius = radius; P.quality_threshold = quality_threshold;
    const dim3 grid(h->n_envs), block(64);
    if (!offsets_dev)
        hipLaunchKernelGGL(k_extract_samples<false>, grid, block, lds, h->stream, h->S, h->cap, which, mask_dev, P, libm_ref(h),
                           (long long *)count_dev, status_dev, (const long long *)nullptr, (double *)nullptr, (double *)nullptr, (double *)nullptr);
    else
        hipLaunchKernelGGL(k_extract_samples<true>, grid, block, lds, h->stream, h->S, h->cap, which, mask_dev, P, libm_ref(h),
                           (long long *)count_dev, status_dev, (const long long *)offsets_dev, samples_dev, outputs_dev, types_dev);
    HIP_TRY(h, hipGetLastError());
    return MESHENV_OK;
}

int meshenv_step_actor_multi(MeshEnv *h, MeshActor *a, int T, float *actions_dev, float *obs_dev, double *reward_dev, uint8_t *done_dev,
                         uint8_t *complete_dev, float *terminal_obs_dev, int auto_reset, int sample, uint64_t seed, uint64_t counter,
                         float *eps_out_dev)
{
    if (!h || !a) return MESHENV_E_ARG;
    if (T <= 0 || !actions_dev || !obs_dev || !reward_dev || !done_dev || !complete_dev)
        return fail_arg(h, "meshenv_step_actor_multi: T > 0 and non-null device pointers are required");
    if (!a->loaded) {
        h->err = "meshenv_step_actor_multi: the actor has no weights loaded";
        return MESHENV_E_STATE;
    }
    if (a->device != h->device || a->stream != h->stream) {
        h->err = "meshenv_step_actor_multi: env and actor must be on the same device and stream (meshenv_set_stream / meshenv_actor_set_stream)";
        return MESHENV_E_STATE;
    }
    const size_t n = (size_t)h->n_envs;
    // step by step: one launch for all T steps measured slower
    for (int t = 0; t < T; t++) {
        const int rc = meshenv_step_actor(h, a, actions_dev + (size_t)t * n * 3, obs_dev + (size_t)t * n * kObsDim, reward_dev + (size_t)t * n,
                                          done_dev + (size_t)t * n, complete_dev + (size_t)t * n,
                                          terminal_obs_dev ? terminal_obs_dev + (size_t)t * n * kObsDim : nullptr, auto_reset, sample, seed,
                                          counter + (uint64_t)t, actions_dev + (size_t)(t + 1) * n * 3,
                                          eps_out_dev ? eps_out_dev + (size_t)t * n * 3 : nullptr);
        if (rc != MESHENV_OK) return rc;
    }
    return MESHENV_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ fused PPO / A2C / TD3 policies
struct MeshPolicy : HandleBase {
    float *buf = nullptr;  // all weights of the loaded policy, one allocation
    PolicyWeights W{};
    WideNet wide{};        // the [400, 300] policy of meshenv_policy_load_widths (hidden2 != 0); its aux block is W.aux
    int kind = -1, hidden = 0, hidden2 = 0, activation = 0;
    bool loaded = false;
    PackTable table{};     // meshenv_policy_bind: the live tensors and where meshenv_policy_refresh packs them
    int n_copies = 0;
    bool live = false;
};

namespace {

typedef void (*PolicyKernel)(PolicyWeights, PolicyArgs);

// the twelve instantiations: [kind][hidden 64 / 128 / 256][activation]
PolicyKernel policy_kernel(int kind, int hidden, int activation)
{
    static const PolicyKernel table[2][3][2] = {
        {{k_policy_forward<64, kPolicyReLU, kPolicyActorCritic>, k_policy_forward<64, kPolicyTanh, kPolicyActorCritic>},
         {k_policy_forward<128, kPolicyReLU, kPolicyActorCritic>, k_policy_forward<128, kPolicyTanh, kPolicyActorCritic>},
         {k_policy_forward<256, kPolicyReLU, kPolicyActorCritic>, k_policy_forward<256, kPolicyTanh, kPolicyActorCritic>}},
        {{k_policy_forward<64, kPolicyReLU, kPolicyDeterministic>, k_policy_forward<64, kPolicyTanh, kPolicyDeterministic>},
         {k_policy_forward<128, kPolicyReLU, kPolicyDeterministic>, k_policy_forward<128, kPolicyTanh, kPolicyDeterministic>},
         {k_policy_forward<256, kPolicyReLU, kPolicyDeterministic>, k_policy_forward<256, kPolicyTanh, kPolicyDeterministic>}}};
    return table[kind][hidden == 64 ? 0 : hidden == 128 ? 1 : 2][activation];
}

const char *kPolicyShapes = "supported policies: kind 0 (actor-critic: pi and vf towers) or 1 (deterministic tanh actor), two hidden "
                            "layers of width 64, 128 or 256, activation 0 (ReLU) or 1 (Tanh), 18 inputs, 3 actions";

// A policy's buffer, in the tensor order of meshenv_policy_bind: the pi tower (w1 b1 w2 b2 wh bh), the actor-critic kind's vf
// tower, then the 16-float aux block.  Its slot, the last, is log_std or sigma; low and high follow at aux + 3 and aux + 6
// (meshenv_policy_load).  The deterministic kind's bind stops before it.
PackLayout policy_layout(int kind, int H)
{
    PackLayout L;
    L.tower(H, 2, kObsDim, kPolInPad / 16, 3, false);
    if (kind == kPolicyActorCritic) L.tower(H, 2, kObsDim, kPolInPad / 16, 1, false);
    L.vector(3, 16);
    return L;
}

const char *kWideShapes = "supported: kind 1 (deterministic tanh actor), activation 0 (ReLU), hidden widths (400, 300), 18 inputs, "
                          "3 actions; meshenv_policy_load takes the uniform widths 64, 128 and 256";

// One [400, 300] network of csrc/meshenv_wide.h over `in` inputs with n_out head columns, in bind order w1 b1 w2 b2 wh bh.
// Layer 2 has 19 tiles for its 300 neurons and the head 19 K groups for its 300 inputs: the four neurons / inputs past 299
// have no source and stay zero; the bias blocks are padded to the tile count.
void wide_tower(PackLayout &L, int in, int n_out)
{
    L.matrix(kWideH1, in, kPolInPad / 16, kWideT1); L.vector(kWideH1, kWideH1);
    L.matrix(kWideH2, kWideH1, kWideG2, kWideT2); L.vector(kWideH2, kWideH2Pad);
    L.matrix(n_out, kWideH2, kWideGH, 1); L.vector(n_out, 16);
}

void point(const float *buf, const PackSlot *s, WideNet &N) { point(buf, s, {&N.w1p, &N.b1, &N.w2p, &N.b2, &N.whp, &N.bh}); }

// The [400, 300] policy's buffer: the actor, then the aux block of policy_layout.
PackLayout wide_policy_layout()
{
    PackLayout L;
    wide_tower(L, kObsDim, 3);
    L.vector(3, 16);
    return L;
}

PackLayout policy_layout(const MeshPolicy *p) { return p->hidden2 ? wide_policy_layout() : policy_layout(p->kind, p->hidden); }

// k_wide_policy / k_wide_target use more dynamic LDS than a launch gets by default when a workgroup has more than 16 rows
template <typename K>
void wide_lds_limit(K kernel)
{
    if (kWideLdsFloats * sizeof(float) > 48 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(kWideLdsFloats * sizeof(float)));
}

// One launch of k_policy_forward.  The pi workgroups run when an action output is asked for, the vf workgroups when a value
// (or a bootstrap terminal value) is.  Arguments are checked by the callers.
int policy_launch(MeshPolicy *p, const char *fn, const PolicyArgs &A)
{
    const bool pi = A.actions || A.buffer_actions || A.log_prob || A.eps_out;
    const bool vf = p->kind == kPolicyActorCritic && (A.value || A.tvalue);
    if (!pi && !vf) return MESHENV_OK;
    PolicyArgs a = A;
    a.tower0 = pi ? 0 : 1;
    const dim3 grid((A.n + kPolEnvs - 1) / kPolEnvs, (pi ? 1 : 0) + (vf ? 1 : 0));
    DeviceGuard guard(p->device);
    if (p->hidden2)
        return launch(p, guard, fn, [&] {
            wide_lds_limit(k_wide_policy);
            hipLaunchKernelGGL(k_wide_policy, dim3((A.n + kWideRows - 1) / kWideRows), dim3(64 * kWideWaves),
                               kWideLdsFloats * sizeof(float), p->stream, p->wide, p->W.aux, a);
        });
    return launch(p, guard, fn, [&] {
        hipLaunchKernelGGL(policy_kernel(p->kind, p->hidden, p->activation), grid, dim3(4 * p->hidden), 0, p->stream, p->W, a);
    });
}

}  // namespace

extern "C" {

int meshenv_policy_create(int device, void *stream, MeshPolicy **out)
{
    return create_handle("meshenv_policy_create", device, stream, out);
}

void meshenv_policy_destroy(MeshPolicy *p) { destroy_handle(p, p ? p->buf : nullptr); }

const char *meshenv_policy_last_error(const MeshPolicy *p) { return last_error(p); }

int meshenv_policy_set_stream(MeshPolicy *p, void *stream) { return set_stream(p, stream); }

// weights in torch.nn.Linear layout ([out][in], row-major), host pointers
int meshenv_policy_load(MeshPolicy *p, int kind, int hidden, int activation, const float *pi_w1, const float *pi_b1,
                        const float *pi_w2, const float *pi_b2, const float *head_w, const float *head_b, const float *vf_w1,
                        const float *vf_b1, const float *vf_w2, const float *vf_b2, const float *value_w, const float *value_b,
                        const float *log_std_or_sigma, const float *low, const float *high)
{
    if (!p) return MESHENV_E_ARG;
    if ((kind != kPolicyActorCritic && kind != kPolicyDeterministic) || (hidden != 64 && hidden != 128 && hidden != 256) ||
        (activation != kPolicyReLU && activation != kPolicyTanh))
        return fail(p, MESHENV_E_ARG, std::string("meshenv_policy_load: unsupported shape; ") + kPolicyShapes);
    const bool ac = kind == kPolicyActorCritic;
    if (!pi_w1 || !pi_b1 || !pi_w2 || !pi_b2 || !head_w || !head_b || !low || !high || (ac && !log_std_or_sigma))
        return fail(p, MESHENV_E_ARG, "meshenv_policy_load: null weight pointer");
    if (ac && (!vf_w1 || !vf_b1 || !vf_w2 || !vf_b2 || !value_w || !value_b))
        return fail(p, MESHENV_E_ARG, "meshenv_policy_load: the actor-critic kind needs the vf tower and value_net");
    if (!ac && (vf_w1 || vf_b1 || vf_w2 || vf_b2 || value_w || value_b))
        return fail(p, MESHENV_E_ARG, "meshenv_policy_load: the deterministic kind has no vf tower (pass NULL)");
    const PackLayout L = policy_layout(kind, hidden);
    const float *src[kPgTensors] = {pi_w1, pi_b1, pi_w2, pi_b2, head_w, head_b};
    int n = 6;
    if (ac)
        for (const float *t : {vf_w1, vf_b1, vf_w2, vf_b2, value_w, value_b}) src[n++] = t;
    src[n++] = log_std_or_sigma;   // NULL (a deterministic policy without sigma) leaves the slot zero
    const size_t o_aux = L.s[L.n - 1].off;
    std::vector<float> h(L.floats, 0.0f);
    pack_host(L, src, h.data());
    for (int i = 0; i < 3; i++) {
        h[o_aux + 3 + i] = low[i];
        h[o_aux + 6 + i] = high[i];
    }
    DeviceGuard guard(p->device);
    if (guard.err != hipSuccess) return fail(p, MESHENV_E_HIP, "meshenv_policy_load: hipSetDevice failed");
    (void)hipStreamSynchronize(p->stream);   // the previous weights may still be in use
    if (p->buf) (void)hipFree(p->buf);
    p->buf = nullptr;
    p->loaded = false;
    p->live = false;       // the copy table points into the buffer that was freed
    if (hipMalloc((void **)&p->buf, h.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(p->buf, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return fail(p, MESHENV_E_HIP, "meshenv_policy_load: upload failed");
    PolicyTower &pi = p->W.pi, &vf = p->W.vf;
    point(p->buf, L.s, {&pi.w1p, &pi.b1, &pi.w2p, &pi.b2, &pi.whp, &pi.bh});
    if (ac) point(p->buf, L.s + 6, {&vf.w1p, &vf.b1, &vf.w2p, &vf.b2, &vf.whp, &vf.bh});
    else vf = pi;   // never read
    p->W.aux = p->buf + o_aux;
    p->kind = kind; p->hidden = hidden; p->hidden2 = 0; p->activation = activation;
    p->loaded = true;
    return MESHENV_OK;
}

int meshenv_policy_load_widths(MeshPolicy *p, int kind, int hidden1, int hidden2, int activation, const float *w1, const float *b1,
                               const float *w2, const float *b2, const float *head_w, const float *head_b, const float *sigma,
                               const float *low, const float *high)
{
    if (!p) return MESHENV_E_ARG;
    if (kind != kPolicyDeterministic || activation != kPolicyReLU || hidden1 != kWideH1 || hidden2 != kWideH2)
        return fail(p, MESHENV_E_ARG, std::string("meshenv_policy_load_widths: unsupported shape; ") + kWideShapes);
    if (!w1 || !b1 || !w2 || !b2 || !head_w || !head_b || !low || !high)
        return fail(p, MESHENV_E_ARG, "meshenv_policy_load_widths: null weight pointer");
    const PackLayout L = wide_policy_layout();
    const float *src[7] = {w1, b1, w2, b2, head_w, head_b, sigma};   // NULL sigma leaves the slot zero
    const size_t o_aux = L.s[L.n - 1].off;
    std::vector<float> h(L.floats, 0.0f);
    pack_host(L, src, h.data());
    for (int i = 0; i < 3; i++) {
        h[o_aux + 3 + i] = low[i];
        h[o_aux + 6 + i] = high[i];
    }
    DeviceGuard guard(p->device);
    if (guard.err != hipSuccess) return fail(p, MESHENV_E_HIP, "meshenv_policy_load_widths: hipSetDevice failed");
    (void)hipStreamSynchronize(p->stream);   // the previous weights may still be in use
    if (p->buf) (void)hipFree(p->buf);
    p->buf = nullptr;
    p->loaded = false;
    p->live = false;
    if (hipMalloc((void **)&p->buf, h.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(p->buf, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return fail(p, MESHENV_E_HIP, "meshenv_policy_load_widths: upload failed");
    point(p->buf, L.s, p->wide);
    p->W.aux = p->buf + o_aux;
    p->kind = kind; p->hidden = hidden1; p->hidden2 = hidden2; p->activation = activation;
    p->loaded = true;
    return MESHENV_OK;
}

int meshenv_policy_forward(MeshPolicy *p, int n, const float *obs_dev, const float *noise_dev, int sample, uint64_t seed,
                           uint64_t counter, float *actions_dev, float *buffer_actions_dev, float *log_prob_dev, float *value_dev,
                           float *eps_out_dev)
{
    if (!p) return MESHENV_E_ARG;
    if (!p->loaded) return fail(p, MESHENV_E_STATE, "meshenv_policy_forward: no weights loaded");
    if (n <= 0 || !obs_dev) return fail(p, MESHENV_E_ARG, "meshenv_policy_forward: n > 0 and obs_dev are required");
    if (noise_dev && sample) return fail(p, MESHENV_E_ARG, "meshenv_policy_forward: explicit noise and sample are exclusive");
    if (p->kind == kPolicyDeterministic && (log_prob_dev || value_dev))
        return fail(p, MESHENV_E_ARG, "meshenv_policy_forward: the deterministic kind has no log_prob / value (pass NULL)");
    if (eps_out_dev && !sample && !noise_dev)
        return fail(p, MESHENV_E_ARG, "meshenv_policy_forward: eps_out_dev without noise");
    const bool pi = actions_dev || buffer_actions_dev || log_prob_dev || eps_out_dev;
    if (!pi && !value_dev) return fail(p, MESHENV_E_ARG, "meshenv_policy_forward: no output requested");
    if (!pi && (noise_dev || sample)) return fail(p, MESHENV_E_ARG, "meshenv_policy_forward: noise without an action output");
    PolicyArgs A{};
    A.n = n; A.obs = obs_dev; A.noise = noise_dev; A.sample = sample ? 1 : 0; A.seed = seed; A.counter = counter;
    A.actions = actions_dev; A.buffer_actions = buffer_actions_dev; A.log_prob = log_prob_dev; A.value = value_dev;
    A.eps_out = eps_out_dev;
    return policy_launch(p, "meshenv_policy_forward", A);
}

int meshenv_step_policy_multi(MeshEnv *h, MeshPolicy *p, int T, float *obs_dev, int sample, uint64_t seed, uint64_t counter,
                              float *actions_dev, float *buffer_actions_dev, float *log_prob_dev, float *value_dev, float *eps_dev,
                              double *reward_dev, uint8_t *done_dev, uint8_t *complete_dev, float *terminal_obs_dev,
                              float *terminal_value_dev, float *last_value_dev, int auto_reset)
{
    if (!h || !p) return MESHENV_E_ARG;
    if (T <= 0 || !obs_dev || !actions_dev || !reward_dev || !done_dev || !complete_dev)
        return fail_arg(h, "meshenv_step_policy_multi: T > 0 and non-null obs, actions, reward, done and complete are required");
    if (!p->loaded) {
        h->err = "meshenv_step_policy_multi: the policy has no weights loaded";
        return MESHENV_E_STATE;
    }
    if (p->device != h->device || p->stream != h->stream) {   // the policy and step launches are ordered by the stream alone
        h->err = "meshenv_step_policy_multi: env and policy must be on the same device and stream (meshenv_set_stream / "
                 "meshenv_policy_set_stream)";
        return MESHENV_E_STATE;
    }
    if (p->kind == kPolicyDeterministic && (log_prob_dev || value_dev || terminal_value_dev || last_value_dev))
        return fail_arg(h, "meshenv_step_policy_multi: the deterministic kind has no log_prob / value outputs (pass NULL)");
    if (eps_dev && !sample) return fail_arg(h, "meshenv_step_policy_multi: eps_dev without sample");
    if (terminal_value_dev && !terminal_obs_dev) return fail_arg(h, "meshenv_step_policy_multi: terminal_value_dev needs terminal_obs_dev");
    MESHENV_ON_DEVICE(h);
    const size_t n = (size_t)h->n_envs;
    PolicyArgs A{};
    A.n = (int)n; A.sample = sample ? 1 : 0; A.seed = seed;
    for (int t = 0; t <= T; t++) {
        // the policy on obs_t (t == T: values only), with the terminal values of step t - 1 in the vf workgroups
        A.obs = obs_dev + (size_t)t * n * kObsDim;
        A.counter = counter + (uint64_t)t;
        const bool last = t == T;
        A.actions = last ? nullptr : actions_dev + (size_t)t * n * 3;
        A.buffer_actions = last || !buffer_actions_dev ? nullptr : buffer_actions_dev + (size_t)t * n * 3;
        A.log_prob = last || !log_prob_dev ? nullptr : log_prob_dev + (size_t)t * n;
        A.eps_out = last || !eps_dev ? nullptr : eps_dev + (size_t)t * n * 3;
        A.value = last ? last_value_dev : value_dev ? value_dev + (size_t)t * n : nullptr;
        A.sample = last ? 0 : (sample ? 1 : 0);
        const bool boot = t > 0 && terminal_value_dev;
        A.tobs = boot ? terminal_obs_dev + (size_t)(t - 1) * n * kObsDim : nullptr;
        A.tdone = boot ? done_dev + (size_t)(t - 1) * n : nullptr;
        A.tcomplete = boot ? complete_dev + (size_t)(t - 1) * n : nullptr;
        A.tvalue = boot ? terminal_value_dev + (size_t)(t - 1) * n : nullptr;
        const int ra = policy_launch(p, "meshenv_step_policy_multi", A);
        if (ra != MESHENV_OK) {
            h->err = p->err;
            return ra;
        }
        if (last) break;
        const int rc = launch_step(h, 1, A.actions, obs_dev + (size_t)(t + 1) * n * kObsDim, reward_dev + (size_t)t * n,
                                   done_dev + (size_t)t * n, complete_dev + (size_t)t * n,
                                   terminal_obs_dev ? terminal_obs_dev + (size_t)t * n * kObsDim : nullptr, auto_reset);
        if (rc != MESHENV_OK) return rc;
    }
    return MESHENV_OK;
}

int meshenv_gae(MeshEnv *h, int T, const double *reward_dev, const float *value_dev, const uint8_t *done_dev,
                const float *terminal_value_dev, const float *last_value_dev, double gamma, double gae_lambda,
                float *advantage_dev, float *return_dev, float *buffer_reward_dev)
{
    if (!h) return MESHENV_E_ARG;
    if (T < 1) return fail_arg(h, "meshenv_gae: T >= 1 is required");
    if (!reward_dev || !value_dev || !done_dev || !last_value_dev || !advantage_dev)
        return fail_arg(h, "meshenv_gae: reward, value, done, last_value and advantage are required");
    if (!(gamma >= 0.0 && gamma <= 1.0) || !(gae_lambda >= 0.0 && gae_lambda <= 1.0))
        return fail_arg(h, "meshenv_gae: gamma and gae_lambda must be finite and in [0, 1]");
    const size_t n = (size_t)h->n_envs, tn = (size_t)T * n;
    struct Range { const void *p; size_t bytes; };
    const Range in[] = {{reward_dev, tn * 8}, {value_dev, tn * 4}, {done_dev, tn}, {terminal_value_dev, tn * 4},
                        {last_value_dev, n * 4}};
    const Range out[] = {{advantage_dev, tn * 4}, {return_dev, tn * 4}, {buffer_reward_dev, tn * 4}};
    auto overlap = [](const Range &x, const Range &y) {
        const uintptr_t a = (uintptr_t)x.p, b = (uintptr_t)y.p;
        return x.p && y.p && a < b + y.bytes && b < a + x.bytes;
    };
    for (int i = 0; i < 3; i++) {
        for (const Range &r : in)
            if (overlap(out[i], r)) return fail_arg(h, "meshenv_gae: an output overlaps an input");
        for (int j = 0; j < i; j++)
            if (overlap(out[i], out[j])) return fail_arg(h, "meshenv_gae: two outputs overlap");
    }
    MESHENV_ON_DEVICE(h);
    GaeArgs A{};
    A.T = T; A.n = h->n_envs;
    A.g = (float)gamma; A.gl = (float)(gamma * gae_lambda);
    A.reward = reward_dev; A.value = value_dev; A.done = done_dev; A.tvalue = terminal_value_dev; A.last_value = last_value_dev;
    A.adv = advantage_dev; A.ret = return_dev; A.brew = buffer_reward_dev;
    const bool long_t = T > kGaeShortT;   // the two workgroup shapes of meshenv_gae.h
    hipLaunchKernelGGL(long_t ? k_gae<512> : k_gae<256>, dim3((unsigned)((n + kGaeEnvs - 1) / kGaeEnvs)), dim3(long_t ? 512 : 256),
                       0, h->stream, A);
    HIP_TRY(h, hipGetLastError());
    return MESHENV_OK;
}

int meshenv_replay_record_floats(void) { return kReplayR; }

int meshenv_replay_add(MeshEnv *h, int T, const float *obs0_dev, const float *obs_after_dev, const float *terminal_obs_dev,
                       const float *actions_dev, const double *reward_dev, const uint8_t *done_dev, const uint8_t *complete_dev,
                       const float *action_low_high_host, int handle_timeouts, float *store_dev, int rows, int pos)
{
    if (!h) return MESHENV_E_ARG;
    if (T < 1) return fail_arg(h, "meshenv_replay_add: T >= 1 is required");
    if (rows < 1) return fail_arg(h, "meshenv_replay_add: rows >= 1 is required");
    if (pos < 0 || pos >= rows) return fail_arg(h, "meshenv_replay_add: pos must be in [0, rows)");
    if (!obs0_dev || !obs_after_dev || !terminal_obs_dev || !actions_dev || !reward_dev || !done_dev || !complete_dev || !store_dev)
        return fail_arg(h, "meshenv_replay_add: obs0, obs_after, terminal_obs, actions, reward, done, complete and store are "
                           "required");
    if ((uintptr_t)store_dev % 16 != 0) return fail_arg(h, "meshenv_replay_add: the store must be 16-byte aligned");
    const size_t n = (size_t)h->n_envs, tn = (size_t)T * n;
    struct Range { const void *p; size_t bytes; };
    const Range store{store_dev, (size_t)rows * n * kReplayR * sizeof(float)};
    const Range in[] = {{obs0_dev, n * kObsDim * 4}, {obs_after_dev, tn * kObsDim * 4}, {terminal_obs_dev, tn * kObsDim * 4},
                        {actions_dev, tn * 3 * 4}, {reward_dev, tn * 8}, {done_dev, tn}, {complete_dev, tn}};
    for (const Range &r : in) {
        const uintptr_t a = (uintptr_t)store.p, b = (uintptr_t)r.p;
        if (a < b + r.bytes && b < a + store.bytes) return fail_arg(h, "meshenv_replay_add: an input overlaps the store");
    }
    MESHENV_ON_DEVICE(h);
    ReplayAddArgs A{};
    A.n = h->n_envs; A.rows = rows; A.T = T;
    A.t0 = T > rows ? T - rows : 0;     // T sequential adds leave the last `rows` steps
    A.row0 = (int)(((long long)pos + A.t0) % rows);
    A.handle_timeouts = handle_timeouts ? 1 : 0;
    if (action_low_high_host) {
        const float *lh = action_low_high_host;
        A.scale = 1;
        A.lo0 = lh[0]; A.lo1 = lh[1]; A.lo2 = lh[2]; A.hi0 = lh[3]; A.hi1 = lh[4]; A.hi2 = lh[5];
    }
    A.obs0 = obs0_dev; A.obs_after = obs_after_dev; A.tobs = terminal_obs_dev; A.actions = actions_dev;
    A.reward = reward_dev; A.done = done_dev; A.complete = complete_dev; A.store = store_dev;
    const int steps = T - A.t0;
    const unsigned gy = (unsigned)((steps + 3) / 4 < 65535 ? (steps + 3) / 4 : 65535);      // a workgroup walks about four steps
    hipLaunchKernelGGL(k_replay_add, dim3((unsigned)((n + kReplayGroups - 1) / kReplayGroups), gy), dim3(kReplayThreads), 0,
                       h->stream, A);
    HIP_TRY(h, hipGetLastError());
    return MESHENV_OK;
}

}  // extern "C"

namespace {

// meshenv_replay_sample (n_batches = 0: one batch, caller indices allowed) and meshenv_replay_sample_batches (n_batches >= 1)
int replay_sample_launch(MeshEnv *h, const std::string &fn, const float *store_dev, int rows, int size, int batch, int n_batches,
                         uint64_t seed, uint64_t counter, const int32_t *rows_in_dev, const int32_t *envs_in_dev, float *obs_out_dev,
                         float *actions_out_dev, float *next_obs_out_dev, float *dones_out_dev, float *rewards_out_dev,
                         int32_t *rows_out_dev, int32_t *envs_out_dev)
{
    auto refuse = [&](const char *msg) { return fail_arg(h, (fn + ": " + msg).c_str()); };
    if (batch < 1) return refuse("batch >= 1 is required");
    if (rows < 1) return refuse("rows >= 1 is required");
    if (size < 1 || size > rows) return refuse("size must be in [1, rows] (an empty buffer has no samples)");
    if (!store_dev || !obs_out_dev || !actions_out_dev || !next_obs_out_dev || !dones_out_dev || !rewards_out_dev)
        return refuse("store and the five outputs are required");
    if ((rows_in_dev != nullptr) != (envs_in_dev != nullptr)) return refuse("rows_in and envs_in are given together or not at all");
    if ((uintptr_t)store_dev % 16 != 0) return refuse("the store must be 16-byte aligned");
    const size_t n = (size_t)h->n_envs, B = (size_t)batch * (size_t)(n_batches > 0 ? n_batches : 1);
    struct Range { const void *p; size_t bytes; };
    const Range in[] = {{store_dev, (size_t)rows * n * kReplayR * sizeof(float)}, {rows_in_dev, B * 4}, {envs_in_dev, B * 4}};
    const Range out[] = {{obs_out_dev, B * kObsDim * 4}, {actions_out_dev, B * 3 * 4}, {next_obs_out_dev, B * kObsDim * 4},
                         {dones_out_dev, B * 4}, {rewards_out_dev, B * 4}, {rows_out_dev, B * 4}, {envs_out_dev, B * 4}};
    auto overlap = [](const Range &x, const Range &y) {
        const uintptr_t a = (uintptr_t)x.p, b = (uintptr_t)y.p;
        return x.p && y.p && a < b + y.bytes && b < a + x.bytes;
    };
    for (int i = 0; i < 7; i++) {
        if (n_batches > 0 && ((uintptr_t)out[i].p & 3) != 0) return refuse("an output is not 4-byte aligned");
        if (overlap(out[i], in[0])) return refuse("an output overlaps the store");
        if (overlap(out[i], in[1]) || overlap(out[i], in[2])) return refuse("an output overlaps rows_in / envs_in");
        for (int j = 0; j < i; j++)
            if (overlap(out[i], out[j])) return refuse("two outputs overlap");
    }
    MESHENV_ON_DEVICE(h);
    ReplaySampleArgs A{};
    A.n = h->n_envs; A.rows = rows; A.size = size; A.B = (int)B;
    A.seed = seed; A.counter = counter;
    A.store = store_dev; A.rows_in = rows_in_dev; A.envs_in = envs_in_dev;
    A.obs = obs_out_dev; A.act = actions_out_dev; A.next = next_obs_out_dev; A.dones = dones_out_dev; A.rew = rewards_out_dev;
    A.rows_out = rows_out_dev; A.envs_out = envs_out_dev;
    const dim3 grid((unsigned)((B + kReplaySamples - 1) / kReplaySamples));
    if (n_batches > 0) hipLaunchKernelGGL(k_replay_sample_batches, grid, dim3(kReplayThreads), 0, h->stream, A, batch);
    else hipLaunchKernelGGL(k_replay_sample, grid, dim3(kReplayThreads), 0, h->stream, A);
    HIP_TRY(h, hipGetLastError());
    return MESHENV_OK;
}

}  // namespace

extern "C" {

int meshenv_replay_sample(MeshEnv *h, const float *store_dev, int rows, int size, int batch, uint64_t seed, uint64_t counter,
                          const int32_t *rows_in_dev, const int32_t *envs_in_dev, float *obs_out_dev, float *actions_out_dev,
                          float *next_obs_out_dev, float *dones_out_dev, float *rewards_out_dev, int32_t *rows_out_dev,
                          int32_t *envs_out_dev)
{
    if (!h) return MESHENV_E_ARG;
    return replay_sample_launch(h, "meshenv_replay_sample", store_dev, rows, size, batch, 0, seed, counter, rows_in_dev, envs_in_dev,
                                obs_out_dev, actions_out_dev, next_obs_out_dev, dones_out_dev, rewards_out_dev, rows_out_dev, envs_out_dev);
}

static_assert(MESHENV_REPLAY_BATCHES_MAX_SAMPLES <= INT32_MAX / kReplayR, "k_replay_sample_batches indexes its samples in int32");

int meshenv_replay_sample_batches(MeshEnv *h, const float *store_dev, int rows, int size, int batch, int n_batches, uint64_t seed,
                                  uint64_t counter, float *obs_out_dev, float *actions_out_dev, float *next_obs_out_dev,
                                  float *dones_out_dev, float *rewards_out_dev, int32_t *rows_out_dev, int32_t *envs_out_dev)
{
    if (!h) return MESHENV_E_ARG;
    if (n_batches < 1) return fail_arg(h, "meshenv_replay_sample_batches: n_batches >= 1 is required");
    if (batch >= 1 && (long long)n_batches * batch > MESHENV_REPLAY_BATCHES_MAX_SAMPLES)
        return fail_arg(h, "meshenv_replay_sample_batches: n_batches * batch exceeds MESHENV_REPLAY_BATCHES_MAX_SAMPLES (2^24)");
    return replay_sample_launch(h, "meshenv_replay_sample_batches", store_dev, rows, size, batch, n_batches, seed, counter, nullptr,
                                nullptr, obs_out_dev, actions_out_dev, next_obs_out_dev, dones_out_dev, rewards_out_dev, rows_out_dev,
                                envs_out_dev);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ policy evaluation
namespace {

// the buffers of a MeshEvalBuffers as kernel arguments; nullptr + message where a required one is missing
const char *eval_args(const MeshEnv *h, const MeshEvalBuffers *b, EvalTallyArgs *A)
{
    if (!b || b->struct_size != (int32_t)sizeof(MeshEvalBuffers)) return "MeshEvalBuffers missing or struct_size mismatch";
    if (!b->target_dev || !b->offset_dev || !b->count_dev || !b->length_dev || !b->seen_dev || !b->return_dev ||
        !b->return_raw_dev || !b->short_dev)
        return "MeshEvalBuffers: a per-env buffer (target, offset, count, length, seen, return, return_raw, short) is NULL";
    if (!b->ep_env_dev || !b->ep_domain_dev || !b->ep_step_dev || !b->ep_length_dev || !b->ep_flags_dev ||
        !b->ep_n_elements_dev || !b->ep_return_dev || !b->ep_return_raw_dev)
        return "MeshEvalBuffers: a per-episode buffer (env, domain, step, length, flags, n_elements, return, return_raw) is NULL";
    const int given = (b->obs_dev ? 1 : 0) + (b->reward_dev ? 1 : 0) + (b->done_dev ? 1 : 0) + (b->complete_dev ? 1 : 0);
    if (given != 0 && given != 4) return "MeshEvalBuffers: obs, reward, done and complete are given all together or not at all";
    EvalTallyArgs a{};
    a.n = h->n_envs;
    a.last_ep = h->S.prm.log_cap > 0 ? h->cold.last_ep : nullptr;
    a.target = b->target_dev; a.offset = b->offset_dev;
    a.count = b->count_dev; a.length = b->length_dev; a.seen = b->seen_dev;
    a.ret = b->return_dev; a.ret_raw = b->return_raw_dev; a.short_envs = b->short_dev;
    a.ep_env = b->ep_env_dev; a.ep_domain = b->ep_domain_dev; a.ep_step = b->ep_step_dev; a.ep_length = b->ep_length_dev;
    a.ep_flags = b->ep_flags_dev; a.ep_n_elem = b->ep_n_elements_dev; a.ep_archive = b->ep_archive_dev;
    a.ep_return = b->ep_return_dev; a.ep_return_raw = b->ep_return_raw_dev; a.ep_quality = b->ep_quality_dev;
    *A = a;
    return nullptr;
}

int eval_check(MeshEnv *h, const char *fn, const MeshEvalBuffers *b, EvalTallyArgs *A)
{
    const char *msg = eval_args(h, b, A);
    if (msg) {
        h->err = std::string(fn) + ": " + msg;
        return MESHENV_E_ARG;
    }
    if (A->ep_quality && h->S.prm.log_cap <= 0) {
        h->err = std::string(fn) + ": ep_quality_dev needs a handle created with log_capacity > 0";
        return MESHENV_E_STATE;
    }
    return MESHENV_OK;
}

int eval_begin_launch(MeshEnv *h, const EvalTallyArgs &A)
{
    MESHENV_ON_DEVICE(h);   // (a no-op inside the entry points, which hold the guard already)
    HIP_TRY(h, hipMemsetAsync(A.short_envs, 0, sizeof(int32_t), h->stream));
    hipLaunchKernelGGL(k_eval_begin, dim3((h->n_envs + 63) / 64), dim3(64), 0, h->stream, h->S, A);
    HIP_TRY(h, hipGetLastError());
    return MESHENV_OK;
}

int eval_tally_launch(MeshEnv *h, EvalTallyArgs A, int step, const double *reward, const uint8_t *done, const uint8_t *complete)
{
    MESHENV_ON_DEVICE(h);   // (a no-op inside the entry points, which hold the guard already)
    A.step = step; A.reward = reward; A.done = done; A.complete = complete;
    hipLaunchKernelGGL(k_eval_tally, dim3((h->n_envs + 63) / 64), dim3(64 * kEvalWaves), 0, h->stream, h->S, A);
    HIP_TRY(h, hipGetLastError());
    if (h->eval_topology) {   // include/meshenv_topology.h: the topology of the meshes this step recorded
        hipLaunchKernelGGL(k_eval_topology, dim3((h->n_envs + 63) / 64), dim3(64 * kEvalWaves), 0, h->stream, h->S, A,
                           h->eval_topology);
        HIP_TRY(h, hipGetLastError());
    }
    return MESHENV_OK;
}

// short_dev -> the pinned host word, then wait for the stream
int eval_read_short(MeshEnv *h, const int32_t *short_dev, int32_t *out)
{
    MESHENV_ON_DEVICE(h);   // (a no-op inside the entry points, which hold the guard already)
    HIP_TRY(h, hipMemcpyAsync(h->eval_host, short_dev, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *out = *h->eval_host;
    return MESHENV_OK;
}

}  // namespace

extern "C" {

int meshenv_eval_begin(MeshEnv *h, const MeshEvalBuffers *bufs)
{
    if (!h) return MESHENV_E_ARG;
    EvalTallyArgs A;
    const int rc = eval_check(h, "meshenv_eval_begin", bufs, &A);
    if (rc != MESHENV_OK) return rc;
    MESHENV_ON_DEVICE(h);
    return eval_begin_launch(h, A);
}

int meshenv_eval_tally(MeshEnv *h, const MeshEvalBuffers *bufs, int step, const double *reward_dev, const uint8_t *done_dev,
                       const uint8_t *complete_dev)
{
    if (!h) return MESHENV_E_ARG;
    if (!reward_dev || !done_dev || !complete_dev) return fail_arg(h, "meshenv_eval_tally: null reward / done / complete");
    EvalTallyArgs A;
    const int rc = eval_check(h, "meshenv_eval_tally", bufs, &A);
    if (rc != MESHENV_OK) return rc;
    MESHENV_ON_DEVICE(h);
    return eval_tally_launch(h, A, step, reward_dev, done_dev, complete_dev);
}

int meshenv_evaluate(MeshEnv *h, MeshPolicy *policy, MeshActor *actor, int sample, uint64_t seed, uint64_t counter, int max_steps,
                     int check_every, const MeshEvalBuffers *bufs, int32_t *steps_out, int32_t *short_out)
{
    if (!h) return MESHENV_E_ARG;
    if ((policy != nullptr) == (actor != nullptr)) return fail_arg(h, "meshenv_evaluate: give exactly one of policy and actor");
    if (max_steps < 1 || check_every < 1) return fail_arg(h, "meshenv_evaluate: max_steps and check_every must be >= 1");
    if (!steps_out || !short_out) return fail_arg(h, "meshenv_evaluate: steps_out and short_out are required");
    if (policy ? !policy->loaded : !actor->loaded) {
        h->err = "meshenv_evaluate: the policy / actor has no weights loaded";
        return MESHENV_E_STATE;
    }
    if (policy ? (policy->device != h->device || policy->stream != h->stream) : (actor->device != h->device || actor->stream != h->stream)) {
        h->err = "meshenv_evaluate: env and policy / actor must be on the same device and stream";
        return MESHENV_E_STATE;
    }
    EvalTallyArgs A;
    int rc = eval_check(h, "meshenv_evaluate", bufs, &A);
    if (rc != MESHENV_OK) return rc;
    MESHENV_ON_DEVICE(h);
    const size_t n = (size_t)h->n_envs;
    // every allocation before the first launch: nothing is allocated on the per-step path
    if (!h->eval_host) {
        void *p = nullptr;
        HIP_TRY(h, hipHostMalloc(&p, sizeof(int32_t), hipHostMallocDefault));
        h->eval_host = (int32_t *)p;
    }
    if (!h->eval_act && (rc = dev_alloc(h, &h->eval_act, 2 * n * 3)) != MESHENV_OK) return rc;
    if (!bufs->obs_dev && !h->eval_obs) {
        if ((rc = dev_alloc(h, &h->eval_obs, n * kObsDim)) != MESHENV_OK || (rc = dev_alloc(h, &h->eval_reward, n)) != MESHENV_OK ||
            (rc = dev_alloc(h, &h->eval_done, n)) != MESHENV_OK || (rc = dev_alloc(h, &h->eval_complete, n)) != MESHENV_OK)
            return rc;
    }
    float *obs = bufs->obs_dev ? bufs->obs_dev : h->eval_obs;
    double *reward = bufs->obs_dev ? bufs->reward_dev : h->eval_reward;
    uint8_t *done = bufs->obs_dev ? bufs->done_dev : h->eval_done;
    uint8_t *complete = bufs->obs_dev ? bufs->complete_dev : h->eval_complete;
    float *act[2] = {h->eval_act, h->eval_act + n * 3};
    *steps_out = 0;
    *short_out = 0;
    if ((rc = meshenv_reset(h, nullptr, obs)) != MESHENV_OK) return rc;
    if ((rc = eval_begin_launch(h, A)) != MESHENV_OK) return rc;
    int32_t short_envs = 0;
    if ((rc = eval_read_short(h, A.short_envs, &short_envs)) != MESHENV_OK) return rc;
    if (short_envs == 0) return MESHENV_OK;
    if (actor && (rc = actor_launch(actor, "meshenv_evaluate", (int)n, obs, nullptr, act[0], sample, seed, counter, nullptr)) != MESHENV_OK) {
        h->err = actor->err;
        return rc;
    }
    PolicyArgs P{};
    P.n = (int)n; P.obs = obs; P.sample = sample ? 1 : 0; P.seed = seed; P.actions = act[0];
    int t = 0;
    while (t < max_steps) {
        if (policy) {
            P.counter = counter + (uint64_t)t;
            if ((rc = policy_launch(policy, "meshenv_evaluate", P)) != MESHENV_OK) {
                h->err = policy->err;
                return rc;
            }
            rc = launch_step(h, 1, act[0], obs, reward, done, complete, nullptr, 1);
        } else {
            rc = meshenv_step_actor(h, actor, act[t & 1], obs, reward, done, complete, nullptr, 1, sample, seed, counter + (uint64_t)t + 1,
                                    act[(t + 1) & 1], nullptr);
        }
        if (rc != MESHENV_OK) return rc;
        if ((rc = eval_tally_launch(h, A, t, reward, done, complete)) != MESHENV_OK) return rc;
        t += 1;
        if (t % check_every == 0 || t == max_steps) {
            if ((rc = eval_read_short(h, A.short_envs, &short_envs)) != MESHENV_OK) return rc;
            if (short_envs == 0) break;
        }
    }
    *steps_out = t;
    *short_out = short_envs;
    return MESHENV_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ SAC / TD3 TD targets
struct MeshTarget : HandleBase {
    int kind = -1;
    float gamma = 0.f, ent_coef = 0.f, policy_noise = 0.f, noise_clip = 0.f;
    float *buf = nullptr;      // every packed weight, one allocation, zeroed once
    TargetWeights W{};
    WideNet wide_actor{}, wide_q{};   // kind 2
    PackTable table{};
    int n_copies = 0;
    bool bound = false, packed = false;
};

namespace {

const char *kTargetKinds = "supported kinds: 0 (SAC: ReLU [128, 128, 128] actor with mu / log_std heads and twin ReLU [128, 128, 128] "
                           "critics), 1 (TD3: ReLU [256, 256] tanh actor and twin ReLU [256, 256] critics) or 2 (DDPG: ReLU [400, 300] "
                           "tanh actor and one ReLU [400, 300] critic); 18 observations, 3 actions";

// The target's buffer, in the tensor order of meshenv_target_bind: the towers actor (SAC: mu at column 0 and log_std at column 3
// of its head tile), q1 and q2, each w1 b1 w2 b2 [w3 b3] wh bh, then log_ent_coef.  Its slot, the last, is there for both
// kinds; a bind without log_ent_coef stops before it.
PackLayout target_layout(int kind)
{
    if (kind == kTargetDDPG) {   // actor and the one critic (csrc/meshenv_wide.h), six tensors each
        PackLayout L;
        wide_tower(L, kObsDim, 3);
        wide_tower(L, kTgtIn, 1);
        return L;
    }
    const bool sac = kind == kTargetSAC;
    const int H = sac ? 128 : 256, NL = sac ? 3 : 2;
    PackLayout L;
    L.tower(H, NL, kObsDim, kPolInPad / 16, 3, sac);
    for (int q = 0; q < 2; q++) L.tower(H, NL, kTgtIn, kPolInPad / 16, 1, false);
    L.vector(1, 4);
    return L;
}

}  // namespace

extern "C" {

int meshenv_target_create(int device, void *stream, int kind, float gamma, float ent_coef, float policy_noise, float noise_clip,
                          MeshTarget **out)
{
    std::string refusal;
    if (kind != kTargetSAC && kind != kTargetTD3 && kind != kTargetDDPG) refusal = std::string("unsupported kind; ") + kTargetKinds;
    else if (!(gamma >= 0.0f && gamma <= 1.0f) || !std::isfinite(ent_coef) || !(policy_noise >= 0.0f) || !(noise_clip >= 0.0f) ||
             !std::isfinite(policy_noise) || !std::isfinite(noise_clip))
        refusal = "gamma must lie in [0, 1], ent_coef be finite, policy_noise and noise_clip be finite and >= 0";
    const int rc = create_handle("meshenv_target_create", device, stream, out, refusal);
    if (rc != MESHENV_OK) return rc;
    MeshTarget *t = *out;
    t->kind = kind;
    t->gamma = gamma; t->ent_coef = ent_coef; t->policy_noise = policy_noise; t->noise_clip = noise_clip;
    return MESHENV_OK;
}

void meshenv_target_destroy(MeshTarget *t) { destroy_handle(t, t ? t->buf : nullptr); }

const char *meshenv_target_last_error(const MeshTarget *t) { return last_error(t); }

int meshenv_target_set_stream(MeshTarget *t, void *stream) { return set_stream(t, stream); }

int meshenv_target_bind(MeshTarget *t, const float *const *actor_dev, int n_actor, const float *const *q1_dev,
                        const float *const *q2_dev, int n_critic, const float *log_ent_coef_dev)
{
    if (!t) return MESHENV_E_ARG;
    const bool sac = t->kind == kTargetSAC, ddpg = t->kind == kTargetDDPG;
    const int NL = sac ? 3 : 2;
    const int want_actor = 2 * NL + (sac ? 4 : 2), want_critic = 2 * NL + 2;
    if (ddpg && q2_dev) return fail(t, MESHENV_E_ARG, "meshenv_target_bind: DDPG has one critic (pass q2_dev = NULL)");
    if (!actor_dev || !q1_dev || (!ddpg && !q2_dev) || n_actor != want_actor || n_critic != want_critic)
        return fail(t, MESHENV_E_ARG, "meshenv_target_bind: kind " + std::to_string(t->kind) + " takes " +
                           std::to_string(want_actor) + " actor and " + std::to_string(want_critic) + " critic tensors; " + kTargetKinds);
    for (int i = 0; i < n_actor; i++)
        if (!actor_dev[i]) return fail(t, MESHENV_E_ARG, "meshenv_target_bind: null actor tensor");
    for (int i = 0; i < n_critic; i++)
        if (!q1_dev[i] || (!ddpg && !q2_dev[i])) return fail(t, MESHENV_E_ARG, "meshenv_target_bind: null critic tensor");
    if (!sac && log_ent_coef_dev)
        return fail(t, MESHENV_E_ARG, "meshenv_target_bind: TD3 / DDPG has no entropy coefficient (pass NULL)");
    DeviceGuard guard(t->device);
    if (guard.err != hipSuccess) return fail(t, MESHENV_E_HIP, "meshenv_target_bind: hipSetDevice failed");
    const PackLayout L = target_layout(t->kind);
    static_assert(10 + 2 * 8 + 1 <= kTgtMaxCopies, "the copy table holds SAC's 27 sources");
    if (!zeroed_once(t, &t->buf, L.floats)) return fail(t, MESHENV_E_HIP, "meshenv_target_bind: allocation failed");
    const float *src[kTgtMaxCopies];
    int n = 0;
    for (int i = 0; i < n_actor; i++) src[n++] = actor_dev[i];
    for (int i = 0; i < n_critic; i++) src[n++] = q1_dev[i];
    for (int i = 0; !ddpg && i < n_critic; i++) src[n++] = q2_dev[i];
    if (log_ent_coef_dev) src[n++] = log_ent_coef_dev;
    t->n_copies = pack_table(L, src, n, t->buf, t->table);
    if (ddpg) {
        point(t->buf, L.s, t->wide_actor);
        point(t->buf, L.s + want_actor, t->wide_q);
        t->bound = true;
        t->packed = false;
        return MESHENV_OK;
    }
    int at = 0;
    for (TargetTower *T : {&t->W.actor, &t->W.q1, &t->W.q2}) {
        T->w3p = T->b3 = nullptr;
        if (NL == 3) point(t->buf, L.s + at, {&T->w1p, &T->b1, &T->w2p, &T->b2, &T->w3p, &T->b3, &T->whp, &T->bh});
        else point(t->buf, L.s + at, {&T->w1p, &T->b1, &T->w2p, &T->b2, &T->whp, &T->bh});
        at += T == &t->W.actor ? want_actor : want_critic;
    }
    t->W.log_ent_coef = log_ent_coef_dev ? t->buf + L.s[at].off : nullptr;
    t->bound = true;
    t->packed = false;
    return MESHENV_OK;
}

int meshenv_target_refresh(MeshTarget *t)
{
    if (!t) return MESHENV_E_ARG;
    if (!t->bound) return fail(t, MESHENV_E_STATE, "meshenv_target_refresh: no tensors bound (meshenv_target_bind)");
    const int rc = pack_refresh(t, "meshenv_target_refresh");
    if (rc == MESHENV_OK) t->packed = true;
    return rc;
}

int meshenv_target_forward(MeshTarget *t, int n, const float *next_obs_dev, const float *rewards_dev, const float *dones_dev,
                           const float *noise_dev, int sample, uint64_t seed, uint64_t counter, float *target_dev,
                           float *next_actions_dev, float *next_log_prob_dev, float *q1_dev, float *q2_dev, float *eps_out_dev)
{
    if (!t) return MESHENV_E_ARG;
    if (!t->packed) return fail(t, MESHENV_E_STATE, "meshenv_target_forward: no weights packed (meshenv_target_bind, then meshenv_target_refresh)");
    if (n <= 0 || !next_obs_dev) return fail(t, MESHENV_E_ARG, "meshenv_target_forward: n > 0 and next_obs_dev are required");
    if (noise_dev && sample) return fail(t, MESHENV_E_ARG, "meshenv_target_forward: explicit noise and sample are exclusive");
    if (target_dev && (!rewards_dev || !dones_dev))
        return fail(t, MESHENV_E_ARG, "meshenv_target_forward: target_dev needs rewards_dev and dones_dev");
    if (t->kind != kTargetSAC && next_log_prob_dev)
        return fail(t, MESHENV_E_ARG, "meshenv_target_forward: TD3 / DDPG has no next_log_prob (pass NULL)");
    if (t->kind == kTargetDDPG && q2_dev)
        return fail(t, MESHENV_E_ARG, "meshenv_target_forward: DDPG has no q2 (pass NULL)");
    if (eps_out_dev && !sample && !noise_dev) return fail(t, MESHENV_E_ARG, "meshenv_target_forward: eps_out_dev without noise");
    if (!target_dev && !next_actions_dev && !next_log_prob_dev && !q1_dev && !q2_dev && !eps_out_dev)
        return fail(t, MESHENV_E_ARG, "meshenv_target_forward: no output requested");
    TargetArgs A{};
    A.n = n; A.next_obs = next_obs_dev; A.rewards = rewards_dev; A.dones = dones_dev; A.noise = noise_dev;
    A.sample = sample ? 1 : 0; A.seed = seed; A.counter = counter;
    A.gamma = t->gamma; A.ent_coef = t->ent_coef; A.policy_noise = t->policy_noise; A.noise_clip = t->noise_clip;
    A.target = target_dev; A.next_actions = next_actions_dev; A.next_log_prob = next_log_prob_dev; A.q1 = q1_dev; A.q2 = q2_dev;
    A.eps_out = eps_out_dev;
    const dim3 grid((n + kTgtRows - 1) / kTgtRows);
    DeviceGuard guard(t->device);
    if (t->kind == kTargetDDPG) {
        WideTargetArgs a{};
        a.n = n; a.next_obs = next_obs_dev; a.rewards = rewards_dev; a.dones = dones_dev; a.noise = noise_dev;
        a.sample = A.sample; a.seed = seed; a.counter = counter;
        a.gamma = t->gamma; a.policy_noise = t->policy_noise; a.noise_clip = t->noise_clip;
        a.target = target_dev; a.next_actions = next_actions_dev; a.q1 = q1_dev; a.eps_out = eps_out_dev;
        return launch(t, guard, "meshenv_target_forward", [&] {
            wide_lds_limit(k_wide_target);
            hipLaunchKernelGGL(k_wide_target, dim3((n + kWideRows - 1) / kWideRows), dim3(64 * kWideWaves),
                               kWideLdsFloats * sizeof(float), t->stream, t->wide_actor, t->wide_q, a);
        });
    }
    return launch(t, guard, "meshenv_target_forward", [&] {
        if (t->kind == kTargetSAC) hipLaunchKernelGGL(k_td_target<kTargetSAC>, grid, dim3(512), 0, t->stream, t->W, A);
        else hipLaunchKernelGGL(k_td_target<kTargetTD3>, grid, dim3(1024), 0, t->stream, t->W, A);
    });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ SAC / TD3 critic loss gradients
struct MeshCriticGrad : GradHandle {
    int kind = -1;
    CgCritic c[2]{};
};

namespace {

template <int H, int NL>
void cg_sizes(int *grads, int *set) { *grads = CgLayout<H, NL>::grads; *set = CgLayout<H, NL>::set; }

void cg_layout(int kind, int *grads, int *set)
{
    if (kind == kTargetSAC) cg_sizes<128, 3>(grads, set);
    else cg_sizes<256, 2>(grads, set);
}

// The workgroups of a gradient kernel on n rows: one per 16-row tile up to 64, then 64, and kCgMaxGroups beyond 512 tiles.
int grad_groups(int n)
{
    const int tiles = (n + kCgRows - 1) / kCgRows;
    return tiles <= 512 ? (tiles < 64 ? tiles : 64) : kCgMaxGroups;
}

// The FNN's kernel strides over its tiles: one workgroup per tile up to kCgMaxGroups.
int fnn_grad_groups(int n)
{
    const int tiles = (n + kCgRows - 1) / kCgRows;
    return tiles < kCgMaxGroups ? tiles : kCgMaxGroups;
}

}  // namespace

extern "C" {

int meshenv_critic_grad_create(int device, void *stream, int kind, MeshCriticGrad **out)
{
    const bool known = kind == kTargetSAC || kind == kTargetTD3;
    const int rc = create_handle("meshenv_critic_grad_create", device, stream, out,
                                 known ? std::string() : std::string("unsupported kind; ") + kCriticGradKinds);
    if (rc == MESHENV_OK) (*out)->kind = kind;
    return rc;
}

void meshenv_critic_grad_destroy(MeshCriticGrad *g) { destroy_handle(g, g ? g->partial : nullptr); }

const char *meshenv_critic_grad_last_error(const MeshCriticGrad *g) { return last_error(g); }

int meshenv_critic_grad_set_stream(MeshCriticGrad *g, void *stream) { return set_stream(g, stream); }

int meshenv_critic_grad_bind(MeshCriticGrad *g, const float *const *q1_dev, const float *const *q2_dev, int n_critic,
                             float *grad_dev, int64_t n_grad)
{
    if (!g) return MESHENV_E_ARG;
    const GradBind &d = kCriticGradBind[g->kind == kTargetSAC ? 0 : 1];
    int grads = 0, set = 0;
    cg_layout(g->kind, &grads, &set);
    const float *const *nets[] = {q1_dev, q2_dev};
    const int counts[] = {n_critic, n_critic};
    const int rc = grad_bind(g, d, nets, counts, grad_dev, n_grad, grads, (size_t)kCgMaxGroups * set);
    if (rc != MESHENV_OK) return rc;
    for (int k = 0; k < 2; k++) grad_bind_pairs(nets[k], n_critic / 2, g->c[k].w, g->c[k].b);
    return MESHENV_OK;
}

int meshenv_critic_grad_backward(MeshCriticGrad *g, int n, const float *obs_dev, const float *actions_dev, const float *target_dev,
                                 float *loss_dev, float *q1_dev, float *q2_dev, float *const *acts1_dev, float *const *acts2_dev)
{
    static const char *fn = "meshenv_critic_grad_backward";
    if (!g) return MESHENV_E_ARG;
    if (!g->bound) return fail(g, MESHENV_E_STATE, std::string(fn) + ": no tensors bound (meshenv_critic_grad_bind)");
    if (n <= 0 || !obs_dev || !actions_dev || !target_dev || !loss_dev)
        return fail(g, MESHENV_E_ARG, std::string(fn) + ": n > 0, obs_dev, actions_dev, target_dev and loss_dev are required");
    if ((acts1_dev == nullptr) != (acts2_dev == nullptr))
        return fail(g, MESHENV_E_ARG, std::string(fn) + ": acts1_dev and acts2_dev go together");
    const int NL = g->kind == kTargetSAC ? 3 : 2;
    for (float *const *acts : {acts1_dev, acts2_dev})
        if (int rc = outputs_ok(g, fn, acts, NL, "activation")) return rc;
    int grads = 0, set = 0;
    cg_layout(g->kind, &grads, &set);
    CgArgs A{};
    A.n = n;
    A.nwg = grad_groups(n);
    A.obs = obs_dev; A.actions = actions_dev; A.target = target_dev;
    A.c[0] = g->c[0]; A.c[1] = g->c[1];
    A.partial = g->partial;
    A.q[0] = q1_dev; A.q[1] = q2_dev;
    for (int l = 0; l < NL; l++) {
        A.acts[0][l] = acts1_dev ? acts1_dev[l] : nullptr;
        A.acts[1][l] = acts2_dev ? acts2_dev[l] : nullptr;
    }
    DeviceGuard guard(g->device);
    return launch_reduced(g, guard, fn, [&] {
        if (g->kind == kTargetSAC) hipLaunchKernelGGL(k_critic_grad<kTargetSAC>, dim3(A.nwg, 2), dim3(512), 0, g->stream, A);
        else hipLaunchKernelGGL(k_critic_grad<kTargetTD3>, dim3(A.nwg, 2 * kCgSplitTD3), dim3(1024), 0, g->stream, A);
    }, [&] {
        hipLaunchKernelGGL(k_critic_grad_reduce, dim3((grads + 255) / 256), dim3(256), 0, g->stream, (const float *)g->partial, A.nwg,
                           set, grads, n, g->grad, loss_dev);
    });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ SAC actor / ent_coef loss gradients
struct MeshActorGrad : GradHandle {
    float ent_coef = 0.0f, target_entropy = 0.0f;
    AgActor a{};
    CgCritic c[2]{};
    const float *log_ent_coef = nullptr;
};

extern "C" {

int meshenv_actor_grad_create(int device, void *stream, float ent_coef, float target_entropy, MeshActorGrad **out)
{
    const bool finite = std::isfinite(ent_coef) && std::isfinite(target_entropy);
    const int rc = create_handle("meshenv_actor_grad_create", device, stream, out,
                                 finite ? "" : "ent_coef and target_entropy must be finite");
    if (rc != MESHENV_OK) return rc;
    (*out)->ent_coef = ent_coef;
    (*out)->target_entropy = target_entropy;
    return MESHENV_OK;
}

void meshenv_actor_grad_destroy(MeshActorGrad *g) { destroy_handle(g, g ? g->partial : nullptr); }

const char *meshenv_actor_grad_last_error(const MeshActorGrad *g) { return last_error(g); }

int meshenv_actor_grad_set_stream(MeshActorGrad *g, void *stream) { return set_stream(g, stream); }

int meshenv_actor_grad_bind(MeshActorGrad *g, const float *const *actor_dev, int n_actor, const float *const *q1_dev,
                            const float *const *q2_dev, int n_critic, const float *log_ent_coef_dev, float *grad_dev, int64_t n_grad)
{
    if (!g) return MESHENV_E_ARG;
    const float *const *nets[] = {actor_dev, q1_dev, q2_dev};
    const int counts[] = {n_actor, n_critic, n_critic};
    const int rc = grad_bind(g, kActorGradBind, nets, counts, grad_dev, n_grad, AgLayout::stride, (size_t)kCgMaxGroups * AgLayout::set);
    if (rc != MESHENV_OK) return rc;
    grad_bind_pairs(actor_dev, 3, g->a.w, g->a.b);
    g->a.mu_w = actor_dev[6]; g->a.mu_b = actor_dev[7]; g->a.ls_w = actor_dev[8]; g->a.ls_b = actor_dev[9];
    for (int k = 0; k < 2; k++) grad_bind_pairs(nets[1 + k], 4, g->c[k].w, g->c[k].b);
    g->log_ent_coef = log_ent_coef_dev;
    return MESHENV_OK;
}

int meshenv_actor_grad_backward(MeshActorGrad *g, int n, const float *obs_dev, const float *noise_dev, int sample, uint64_t seed,
                                uint64_t counter, float *losses_dev, float *eps_out_dev, float *const *parts_dev, float *const *acts_dev)
{
    static const char *fn = "meshenv_actor_grad_backward";
    if (!g) return MESHENV_E_ARG;
    if (!g->bound) return fail(g, MESHENV_E_STATE, std::string(fn) + ": no tensors bound (meshenv_actor_grad_bind)");
    if (n <= 0 || !obs_dev || !losses_dev) return fail(g, MESHENV_E_ARG, std::string(fn) + ": n > 0, obs_dev and losses_dev are required");
    if (noise_dev && sample) return fail(g, MESHENV_E_ARG, std::string(fn) + ": noise_dev and sample are exclusive");
    if (eps_out_dev && !noise_dev && !sample) return fail(g, MESHENV_E_ARG, std::string(fn) + ": eps_out_dev needs noise_dev or sample");
    if (int rc = outputs_ok(g, fn, parts_dev, kAgParts, "per-sample")) return rc;
    if (int rc = outputs_ok(g, fn, acts_dev, 9, "activation")) return rc;
    AgArgs A{};
    A.n = n;
    A.nwg = grad_groups(n);
    A.obs = obs_dev; A.noise = noise_dev; A.sample = sample ? 1 : 0; A.seed = seed; A.counter = counter;
    A.a = g->a; A.c[0] = g->c[0]; A.c[1] = g->c[1];
    A.log_ent_coef = g->log_ent_coef; A.ent_coef = g->ent_coef; A.target_entropy = g->target_entropy;
    A.partial = g->partial;
    A.eps_out = eps_out_dev;
    if (parts_dev) {
        A.actions = parts_dev[0]; A.log_prob = parts_dev[1]; A.q[0] = parts_dev[2]; A.q[1] = parts_dev[3];
        A.dq_da = parts_dev[4]; A.d_mu = parts_dev[5]; A.d_ls = parts_dev[6];
    }
    for (int i = 0; acts_dev && i < 9; i++) A.acts[i / 3][i % 3] = acts_dev[i];
    DeviceGuard guard(g->device);
    return launch_reduced(g, guard, fn, [&] { hipLaunchKernelGGL(k_actor_grad, dim3(A.nwg), dim3(512), 0, g->stream, A); }, [&] {
        hipLaunchKernelGGL(k_actor_grad_reduce, dim3((AgLayout::ent + 255) / 256), dim3(256), 0, g->stream, (const float *)g->partial,
                           A.nwg, n, g->log_ent_coef, g->grad, losses_dev);
    });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ TD3 / DDPG actor loss gradients
static_assert(MESHENV_TD3_ACTOR_GRAD_FLOATS == TaLayout::stride, "include/meshenv_td3_actor_grad.h and csrc/meshenv_td3_actor_grad.h disagree");

struct MeshTd3ActorGrad : GradHandle {
    const float *w[3]{}, *b[3]{};   // the actor
    CgCritic c{};                   // the first critic
};

extern "C" {

int meshenv_td3_actor_grad_create(int device, void *stream, MeshTd3ActorGrad **out)
{
    return create_handle("meshenv_td3_actor_grad_create", device, stream, out);
}

void meshenv_td3_actor_grad_destroy(MeshTd3ActorGrad *g) { destroy_handle(g, g ? g->partial : nullptr); }

const char *meshenv_td3_actor_grad_last_error(const MeshTd3ActorGrad *g) { return last_error(g); }

int meshenv_td3_actor_grad_set_stream(MeshTd3ActorGrad *g, void *stream) { return set_stream(g, stream); }

int meshenv_td3_actor_grad_bind(MeshTd3ActorGrad *g, const float *const *actor_dev, int n_actor, const float *const *q1_dev,
                                int n_critic, float *grad_dev, int64_t n_grad)
{
    if (!g) return MESHENV_E_ARG;
    const float *const *nets[] = {actor_dev, q1_dev};
    const int counts[] = {n_actor, n_critic};
    const int rc = grad_bind(g, kTd3ActorGradBind, nets, counts, grad_dev, n_grad, TaLayout::stride, (size_t)kCgMaxGroups * TaLayout::set);
    if (rc != MESHENV_OK) return rc;
    grad_bind_pairs(actor_dev, 3, g->w, g->b);
    grad_bind_pairs(q1_dev, 3, g->c.w, g->c.b);
    return MESHENV_OK;
}

int meshenv_td3_actor_grad_backward(MeshTd3ActorGrad *g, int n, const float *obs_dev, float *loss_dev, float *const *parts_dev,
                                    float *const *acts_dev)
{
    static const char *fn = "meshenv_td3_actor_grad_backward";
    if (!g) return MESHENV_E_ARG;
    if (!g->bound) return fail(g, MESHENV_E_STATE, std::string(fn) + ": no tensors bound (meshenv_td3_actor_grad_bind)");
    if (n <= 0 || n > (1 << 24) - 16 || !obs_dev || !loss_dev)   // the kernel's 32-bit offsets reach row * 256
        return fail(g, MESHENV_E_ARG, std::string(fn) + ": 0 < n <= 2^24 - 16, obs_dev and loss_dev are required");
    if (int rc = outputs_ok(g, fn, parts_dev, kTaParts, "per-sample")) return rc;
    if (int rc = outputs_ok(g, fn, acts_dev, 4, "activation")) return rc;
    TaArgs A{};
    A.n = n;
    A.nwg = grad_groups(n);
    A.obs = obs_dev;
    for (int l = 0; l < 3; l++) {
        A.w[l] = g->w[l];
        A.b[l] = g->b[l];
    }
    A.c = g->c;
    A.partial = g->partial;
    if (parts_dev) {
        A.actions = parts_dev[0]; A.q = parts_dev[1]; A.dq_da = parts_dev[2]; A.d_pre = parts_dev[3];
    }
    for (int i = 0; acts_dev && i < 4; i++) A.acts[i / 2][i % 2] = acts_dev[i];
    DeviceGuard guard(g->device);
    return launch_reduced(g, guard, fn, [&] { hipLaunchKernelGGL(k_td3_actor_grad, dim3(A.nwg, kCgSplitTD3), dim3(1024), 0, g->stream, A); }, [&] {
        hipLaunchKernelGGL(k_td3_actor_grad_reduce, dim3((TaLayout::params + 255) / 256), dim3(256), 0, g->stream,
                           (const float *)g->partial, A.nwg, n, g->grad, loss_dev);
    });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ DDPG [400, 300] loss gradients
static_assert(MESHENV_DDPG_GRAD_ACTOR_FLOATS == WgActor::stride && MESHENV_DDPG_GRAD_CRITIC_FLOATS == WgCritic::stride &&
              MESHENV_DDPG_GRAD_MAX_ROWS == kWgMaxRows, "include/meshenv_ddpg_grad.h and csrc/meshenv_wide_grad.h disagree");

// (MeshDdpgGrad and the helpers that run under its entry points' device guard stand with the shared handle code, above)
extern "C" {

int meshenv_ddpg_grad_create(int device, void *stream, float loss_scale, MeshDdpgGrad **out)
{
    const bool ok = loss_scale == 0.5f || loss_scale == 1.0f;
    const int rc = create_handle("meshenv_ddpg_grad_create", device, stream, out,
                                 ok ? std::string() : "loss_scale must be 0.5 or 1.0, got " + std::to_string(loss_scale));
    if (rc == MESHENV_OK) (*out)->loss_scale = loss_scale;
    return rc;
}

void meshenv_ddpg_grad_destroy(MeshDdpgGrad *g) { destroy_handle(g, g ? g->space : nullptr); }

const char *meshenv_ddpg_grad_last_error(const MeshDdpgGrad *g) { return last_error(g); }

int meshenv_ddpg_grad_set_stream(MeshDdpgGrad *g, void *stream) { return set_stream(g, stream); }

int meshenv_ddpg_grad_bind(MeshDdpgGrad *g, const float *const *actor_dev, int n_actor, const float *const *q1_dev, int n_critic,
                           float *grad_dev, int64_t n_grad)
{
    if (!g) return MESHENV_E_ARG;
    const float *const *nets[] = {actor_dev, q1_dev};
    const int counts[] = {n_actor, n_critic};
    const std::string refusal = grad_bind_refusal(kDdpgGradBind, nets, counts, grad_dev, n_grad, MESHENV_DDPG_GRAD_FLOATS);
    if (!refusal.empty()) return fail(g, MESHENV_E_ARG, refusal);
    grad_bind_pairs(actor_dev, 3, g->a.w, g->a.b);
    grad_bind_pairs(q1_dev, 3, g->c.w, g->c.b);
    g->grad = grad_dev;
    g->bound = true;
    return MESHENV_OK;
}

int meshenv_ddpg_grad_critic_backward(MeshDdpgGrad *g, int n, const float *obs_dev, const float *actions_dev, const float *y_dev,
                                      float *loss_dev, float *const *parts_dev)
{
    static const char *fn = "meshenv_ddpg_grad_critic_backward";
    if (!g) return MESHENV_E_ARG;
    if (!g->bound) return fail(g, MESHENV_E_STATE, std::string(fn) + ": no tensors bound (meshenv_ddpg_grad_bind)");
    if (n <= 0 || n > kWgMaxRows)
        return fail(g, MESHENV_E_ARG, std::string(fn) + ": 0 < n <= " + std::to_string(kWgMaxRows) + " (MESHENV_DDPG_GRAD_MAX_ROWS), got " +
                       std::to_string(n));
    if (!obs_dev || !actions_dev || !y_dev || !loss_dev)
        return fail(g, MESHENV_E_ARG, std::string(fn) + ": obs_dev, actions_dev, y_dev and loss_dev are required");
    WgCriticArgs A{};
    A.n = n;
    A.two_scale = 2.0f * g->loss_scale;
    A.obs = obs_dev; A.actions = actions_dev; A.target = y_dev;
    A.c = g->c;
    if (int rc = outputs_ok(g, fn, parts_dev, 3, "per-sample")) return rc;
    if (parts_dev) {
        A.q = parts_dev[0]; A.acts[0] = parts_dev[1]; A.acts[1] = parts_dev[2];
    }
    DeviceGuard guard(g->device);
    if (guard.err != hipSuccess) return fail(g, MESHENV_E_HIP, std::string(fn) + ": hipSetDevice failed");
    int rc = wg_reserve(g, n, fn);
    if (rc != MESHENV_OK) return rc;
    float *partial = nullptr;
    A.ws = wg_space(g, wg_rows16(n), &partial);
    rc = launch(g, guard, fn, [&] {
        hipLaunchKernelGGL(k_wgrad_critic_rows, dim3(wg_rows16(n) / kCgRows), dim3(64 * kWideWaves), 0, g->stream, A);
    }, "row phase launch");
    if (rc != MESHENV_OK) return rc;
    return wg_weights<kWgIn, 1>(g, guard, fn, A.ws, partial, n, g->loss_scale, g->grad + WgActor::stride, loss_dev);
}

int meshenv_ddpg_grad_actor_backward(MeshDdpgGrad *g, int n, const float *obs_dev, float *loss_dev, float *const *parts_dev,
                                     float *const *acts_dev)
{
    static const char *fn = "meshenv_ddpg_grad_actor_backward";
    if (!g) return MESHENV_E_ARG;
    if (!g->bound) return fail(g, MESHENV_E_STATE, std::string(fn) + ": no tensors bound (meshenv_ddpg_grad_bind)");
    if (n <= 0 || n > kWgMaxRows)
        return fail(g, MESHENV_E_ARG, std::string(fn) + ": 0 < n <= " + std::to_string(kWgMaxRows) + " (MESHENV_DDPG_GRAD_MAX_ROWS), got " +
                       std::to_string(n));
    if (!obs_dev || !loss_dev) return fail(g, MESHENV_E_ARG, std::string(fn) + ": obs_dev and loss_dev are required");
    WgActorArgs A{};
    A.n = n;
    A.obs = obs_dev;
    A.a = g->a;
    A.c = g->c;
    if (int rc = outputs_ok(g, fn, parts_dev, kTaParts, "per-sample")) return rc;
    if (int rc = outputs_ok(g, fn, acts_dev, 4, "activation")) return rc;
    if (parts_dev) {
        A.actions = parts_dev[0]; A.q = parts_dev[1]; A.dq_da = parts_dev[2]; A.d_pre = parts_dev[3];
    }
    for (int i = 0; acts_dev && i < 4; i++) A.acts[i / 2][i % 2] = acts_dev[i];
    DeviceGuard guard(g->device);
    if (guard.err != hipSuccess) return fail(g, MESHENV_E_HIP, std::string(fn) + ": hipSetDevice failed");
    int rc = wg_reserve(g, n, fn);
    if (rc != MESHENV_OK) return rc;
    float *partial = nullptr;
    A.ws = wg_space(g, wg_rows16(n), &partial);
    rc = launch(g, guard, fn, [&] {
        hipLaunchKernelGGL(k_wgrad_actor_rows, dim3(wg_rows16(n) / kCgRows), dim3(64 * kWideWaves), 0, g->stream, A);
    }, "row phase launch");
    if (rc != MESHENV_OK) return rc;
    return wg_weights<kWgObs, 3>(g, guard, fn, A.ws, partial, n, -1.0f, g->grad, loss_dev);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ PPO / A2C loss gradients
static_assert(MESHENV_PPO_GRAD_FLOATS_64 == PgLayout<64>::stride && MESHENV_PPO_GRAD_FLOATS_128 == PgLayout<128>::stride,
              "include/meshenv_ppo_grad.h and csrc/meshenv_ppo_grad.h disagree");
static_assert(MESHENV_PPO_GRAD_OUTPUTS == kPgOut && MESHENV_PPO_GRAD_PARTS == kPgParts, "include/meshenv_ppo_grad.h and csrc/meshenv_ppo_grad.h disagree");

struct MeshPpoGrad : GradHandle {   // partial: the sets of the widest layout, then the advantage statistics
    PgTower t[2]{};
    const float *log_std = nullptr;
    int hidden = 0, activation = 0;
};

namespace {

typedef void (*PpoGradKernel)(PgArgs);

// the four instantiations: [hidden 64 / 128][activation]
PpoGradKernel ppo_grad_kernel(int hidden, int activation)
{
    static const PpoGradKernel table[2][2] = {{k_ppo_grad<64, kPolicyReLU>, k_ppo_grad<64, kPolicyTanh>},
                                              {k_ppo_grad<128, kPolicyReLU>, k_ppo_grad<128, kPolicyTanh>}};
    return table[hidden == 64 ? 0 : 1][activation];
}

}  // namespace

extern "C" {

int meshenv_ppo_grad_create(int device, void *stream, MeshPpoGrad **out)
{
    return create_handle("meshenv_ppo_grad_create", device, stream, out);
}

void meshenv_ppo_grad_destroy(MeshPpoGrad *g) { destroy_handle(g, g ? g->partial : nullptr); }

const char *meshenv_ppo_grad_last_error(const MeshPpoGrad *g) { return last_error(g); }

int meshenv_ppo_grad_set_stream(MeshPpoGrad *g, void *stream) { return set_stream(g, stream); }

int meshenv_ppo_grad_bind(MeshPpoGrad *g, int hidden, int activation, const float *const *tensors_dev, int n_tensors,
                          float *grad_dev, int64_t n_grad)
{
    if (!g) return MESHENV_E_ARG;
    if (hidden == 256)
        return fail(g, MESHENV_E_ARG, std::string("meshenv_ppo_grad_bind: width 256 is not supported (its dW_2 needs the column split "
                                                  "of the TD3 critic kernel); ") + kPpoGradShapes);
    if ((hidden != 64 && hidden != 128) || (activation != kPolicyReLU && activation != kPolicyTanh))
        return fail(g, MESHENV_E_ARG, std::string("meshenv_ppo_grad_bind: unsupported shape; ") + kPpoGradShapes);
    // the description takes over behind the shape: a width picks its row
    const int want = hidden == 64 ? PgLayout<64>::stride : PgLayout<128>::stride;
    const int rc = grad_bind(g, kPpoGradBind[hidden == 64 ? 0 : 1], &tensors_dev, &n_tensors, grad_dev, n_grad, want,
                             (size_t)kCgMaxGroups * PgLayout<128>::set + 64);
    if (rc != MESHENV_OK) return rc;
    for (int tower = 0; tower < 2; tower++) grad_bind_pairs(tensors_dev + 6 * tower, 3, g->t[tower].w, g->t[tower].b);
    g->log_std = tensors_dev[12];
    g->hidden = hidden;
    g->activation = activation;
    return MESHENV_OK;
}

int meshenv_ppo_grad_backward(MeshPpoGrad *g, int n, const float *obs_dev, const float *actions_dev, const float *old_log_prob_dev,
                              const float *advantages_dev, const float *returns_dev, int a2c, double clip_range, float ent_coef,
                              float vf_coef, int normalize_advantage, int clip_grad, float max_grad_norm, float *out_dev,
                              float *const *parts_dev, float *const *acts_dev)
{
    static const char *fn = "meshenv_ppo_grad_backward";
    if (!g) return MESHENV_E_ARG;
    if (!g->bound) return fail(g, MESHENV_E_STATE, std::string(fn) + ": no tensors bound (meshenv_ppo_grad_bind)");
    if (n <= 0 || n > (1 << 24) - 16 || !obs_dev || !actions_dev || !advantages_dev || !returns_dev || !out_dev)   // 32-bit offsets reach row * 128
        return fail(g, MESHENV_E_ARG, std::string(fn) + ": 0 < n <= 2^24 - 16 and obs, actions, advantages, returns and out are required");
    if (!a2c && !old_log_prob_dev) return fail(g, MESHENV_E_ARG, std::string(fn) + ": PPO's loss needs old_log_prob_dev");
    if (!std::isfinite(clip_range) || !std::isfinite(ent_coef) || !std::isfinite(vf_coef) || !std::isfinite(max_grad_norm) ||
        (!a2c && !(clip_range > 0.0)) || (clip_grad && !(max_grad_norm > 0.0f)))
        return fail(g, MESHENV_E_ARG, std::string(fn) + ": clip_range and max_grad_norm must be finite and > 0, ent_coef and vf_coef finite");
    if (int rc = outputs_ok(g, fn, parts_dev, kPgParts, "per-row")) return rc;
    if (int rc = outputs_ok(g, fn, acts_dev, 4, "activation")) return rc;
    const int H = g->hidden;
    const int set = H == 64 ? PgLayout<64>::set : PgLayout<128>::set, stride = H == 64 ? PgLayout<64>::stride : PgLayout<128>::stride;
    const int params = H == 64 ? PgLayout<64>::params : PgLayout<128>::params;
    float *stats = g->partial + (size_t)kCgMaxGroups * PgLayout<128>::set;
    PgArgs A{};
    A.n = n;
    A.nwg = grad_groups(n);
    A.a2c = a2c ? 1 : 0;
    A.normalize = normalize_advantage && n > 1 ? 1 : 0;
    A.obs = obs_dev; A.actions = actions_dev; A.old_log_prob = old_log_prob_dev; A.adv = advantages_dev; A.returns = returns_dev;
    A.stats = stats;
    // torch clamps a float32 tensor against the Python floats 1 - clip_range and 1 + clip_range, formed in double and then
    // rounded to float32, and compares |ratio - 1| with float32(clip_range): clip_range arrives as the double SB3 holds
    A.lo = (float)(1.0 - clip_range); A.hi = (float)(1.0 + clip_range); A.clip = (float)clip_range; A.vf_coef = vf_coef;
    A.t[0] = g->t[0]; A.t[1] = g->t[1];
    A.log_std = g->log_std;
    A.partial = g->partial;
    if (parts_dev) {
        A.log_prob = parts_dev[0]; A.ratio = parts_dev[1]; A.values = parts_dev[2]; A.advn = parts_dev[3]; A.pass = parts_dev[4];
    }
    for (int i = 0; acts_dev && i < 4; i++) A.acts[i / 2][i % 2] = acts_dev[i];
    DeviceGuard guard(g->device);
    int rc = MESHENV_OK;
    if (A.normalize) {
        rc = launch(g, guard, fn, [&] {
            hipLaunchKernelGGL(k_ppo_adv_stats, dim3(1), dim3(kPgStatThreads), 0, g->stream, advantages_dev, n, stats);
        }, "statistics launch");
        if (rc != MESHENV_OK) return rc;
    }
    rc = launch(g, guard, fn, [&] {
        hipLaunchKernelGGL(ppo_grad_kernel(H, g->activation), dim3(A.nwg, 2), dim3(4 * H), 0, g->stream, A);
    });
    if (rc != MESHENV_OK) return rc;
    rc = launch(g, guard, fn, [&] {
        hipLaunchKernelGGL(k_ppo_grad_reduce, dim3((params + 255) / 256), dim3(256), 0, g->stream, (const float *)g->partial, A.nwg, set,
                           stride, params, n, ent_coef, vf_coef, g->log_std, clip_grad ? 1 : 0, g->grad, out_dev);
    }, "reduction launch");
    if (rc != MESHENV_OK || !clip_grad) return rc;
    return launch(g, guard, fn, [&] {
        hipLaunchKernelGGL(k_ppo_grad_clip, dim3(1), dim3(kPgStatThreads), 0, g->stream, g->grad, H, max_grad_norm, out_dev);
    }, "clip launch");
}

// ---- live weights into a loaded FusedPolicy (the on-policy twin of meshenv_target_bind / meshenv_target_refresh)
int meshenv_policy_bind(MeshPolicy *p, const float *const *tensors_dev, int n_tensors)
{
    if (!p) return MESHENV_E_ARG;
    if (!p->loaded) return fail(p, MESHENV_E_STATE, "meshenv_policy_bind: no weights loaded (meshenv_policy_load lays the buffer out)");
    const bool ac = p->kind == kPolicyActorCritic;
    const int want = ac ? kPgTensors : 6;
    if (!tensors_dev || n_tensors != want)
        return fail(p, MESHENV_E_ARG, "meshenv_policy_bind: the " + std::string(ac ? "actor-critic" : "deterministic") + " kind takes " +
                       std::to_string(want) + " tensors (pi w1 b1 w2 b2 wh bh" + (ac ? ", vf likewise, log_std)" : ")"));
    for (int i = 0; i < want; i++)
        if (!tensors_dev[i]) return fail(p, MESHENV_E_ARG, "meshenv_policy_bind: null tensor");
    static_assert(kPgTensors <= kTgtMaxCopies, "the copy table holds the 13 sources");
    p->n_copies = pack_table(policy_layout(p), tensors_dev, want, p->buf, p->table);
    p->live = true;
    return MESHENV_OK;
}

int meshenv_policy_refresh(MeshPolicy *p)
{
    if (!p) return MESHENV_E_ARG;
    if (!p->loaded || !p->live) return fail(p, MESHENV_E_STATE, "meshenv_policy_refresh: no tensors bound (meshenv_policy_bind)");
    return pack_refresh(p, "meshenv_policy_refresh");
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ Adam steps and polyak_update
static_assert(sizeof(MeshOptimScalars) == sizeof(OptScalars), "include/meshenv_optim.h and csrc/meshenv_optim.h disagree");
static_assert(MESHENV_OPTIM_BLOCKS == kOptBlocks && MESHENV_OPTIM_CHUNK == kOptChunk, "include/meshenv_optim.h and csrc/meshenv_optim.h disagree");
static_assert(MESHENV_OPTIM_ADAM == kOptAdam && MESHENV_OPTIM_POLYAK == kOptPolyak && MESHENV_OPTIM_ADAM_POLYAK == kOptAdamPolyak, "ops");
static_assert(MESHENV_OPTIM_RMSPROP == kOptRmsprop, "ops");

struct OptProgram {
    char *dev = nullptr;        // the segment table, then the job table
    char *host = nullptr;       // pinned staging of the same layout
    size_t cap = 0;
    size_t jobs_at = 0;         // byte offset of the job table
    int n_jobs = 0;
    int n_seg = 0;
    hipEvent_t copied = nullptr;   // the last upload from `host`
    hipStream_t ordered = nullptr; // the stream that is known to be ordered after that upload
    bool bound = false;
};

struct MeshOptim : HandleBase {
    hipStream_t last_stream = nullptr;   // the stream of the last upload or launch: what may still read a table
    bool used = false;
    OptProgram prog[MESHENV_OPTIM_PROGRAMS];
};

namespace {

// The launch of a bound program: k_optim_step, or with a gate (meshenv_onpolicy_train_run) k_optim_step_gated, or with a note
// (meshenv_offpolicy_train_run) k_optim_step_noted, or with a gate and a count (meshenv_onpolicy_learn_run, which passes no
// scalars) k_optim_step_counted, over the same tables.  A noted program must not step what the note reads: the caller has
// looked (optim_program_writes).
int optim_step_launch(MeshOptim *o, int program, const MeshOptimScalars *scalars, const TrainGate *gate, const char *fn,
                      const OptNote *note = nullptr, const OptCounted *counted = nullptr)
{
    if (!o) return MESHENV_E_ARG;
    if (program < 0 || program >= MESHENV_OPTIM_PROGRAMS || (!scalars && !(counted && gate)))
        return fail(o, MESHENV_E_ARG, std::string(fn) + ": program out of range or no scalars");
    OptProgram &P = o->prog[program];
    if (!P.bound) return fail(o, MESHENV_E_STATE, std::string(fn) + ": program " + std::to_string(program) + " is not bound (meshenv_optim_bind)");
    DeviceGuard guard(o->device);
    if (guard.err != hipSuccess) return fail(o, MESHENV_E_HIP, std::string(fn) + ": hipSetDevice failed");
    if (P.ordered != o->stream) {           // the tables were uploaded on another stream: order this one after the upload
        if (hipStreamWaitEvent(o->stream, P.copied, 0) != hipSuccess)
            return fail(o, MESHENV_E_HIP, std::string(fn) + ": hipStreamWaitEvent failed");
        P.ordered = o->stream;
    }
    o->last_stream = o->stream;
    OptScalars S{};
    if (scalars) std::memcpy(&S, scalars, sizeof(S));
    return launch(o, guard, fn, [&] {
        if (counted)
            hipLaunchKernelGGL(k_optim_step_counted, dim3(P.n_jobs), dim3(kOptThreads), 0, o->stream, (const OptSeg *)P.dev,
                               (const OptJob *)(P.dev + P.jobs_at), *counted, *gate);
        else if (note)
            hipLaunchKernelGGL(k_optim_step_noted, dim3(P.n_jobs), dim3(kOptThreads), 0, o->stream, (const OptSeg *)P.dev,
                               (const OptJob *)(P.dev + P.jobs_at), S, *note);
        else if (gate)
            hipLaunchKernelGGL(k_optim_step_gated, dim3(P.n_jobs), dim3(kOptThreads), 0, o->stream, (const OptSeg *)P.dev,
                               (const OptJob *)(P.dev + P.jobs_at), S, *gate);
        else
            hipLaunchKernelGGL(k_optim_step, dim3(P.n_jobs), dim3(kOptThreads), 0, o->stream, (const OptSeg *)P.dev,
                               (const OptJob *)(P.dev + P.jobs_at), S);
    });
}

// The segment of a bound program that writes `ptr` (as a parameter or as a Polyak target), or -1: the host copy of its table.
int optim_program_writes(const MeshOptim *o, int program, const float *ptr)
{
    const OptProgram &P = o->prog[program];
    const OptSeg *segs = reinterpret_cast<const OptSeg *>(P.host);
    for (int i = 0; i < P.n_seg; i++)
        if (segs[i].p == ptr || segs[i].t == ptr) return i;
    return -1;
}

}  // namespace

extern "C" {

int meshenv_optim_create(int device, void *stream, MeshOptim **out)
{
    return create_handle("meshenv_optim_create", device, stream, out);
}

void meshenv_optim_destroy(MeshOptim *o)
{
    if (!o) return;
    DeviceGuard guard(o->device);
    if (o->used) (void)hipStreamSynchronize(o->last_stream);
    for (OptProgram &P : o->prog) {
        if (P.copied) (void)hipEventDestroy(P.copied);
        if (P.dev) (void)hipFree(P.dev);
        if (P.host) (void)hipHostFree(P.host);
    }
    delete o;
}

const char *meshenv_optim_last_error(const MeshOptim *o) { return last_error(o); }

int meshenv_optim_set_stream(MeshOptim *o, void *stream) { return set_stream(o, stream); }

int meshenv_optim_bind(MeshOptim *o, int program, int n_seg, float *const *param_dev, const float *const *grad_dev,
                       float *const *exp_avg_dev, float *const *exp_avg_sq_dev, float *const *target_dev, const int64_t *n,
                       const int32_t *op, const int32_t *block, const int32_t *vec)
{
    if (!o) return MESHENV_E_ARG;
    if (program < 0 || program >= MESHENV_OPTIM_PROGRAMS)
        return fail(o, MESHENV_E_ARG, "meshenv_optim_bind: program " + std::to_string(program) + " out of range");
    if (n_seg < 1 || !param_dev || !grad_dev || !exp_avg_dev || !exp_avg_sq_dev || !target_dev || !n || !op || !block || !vec)
        return fail(o, MESHENV_E_ARG, "meshenv_optim_bind: n_seg > 0 and all nine arrays are required");
    int64_t n_jobs = 0;
    for (int i = 0; i < n_seg; i++) {
        const std::string at = "meshenv_optim_bind: segment " + std::to_string(i) + ": ";
        if (op[i] != kOptAdam && op[i] != kOptPolyak && op[i] != kOptAdamPolyak && op[i] != kOptRmsprop)
            return fail(o, MESHENV_E_ARG, at + "op " + std::to_string(op[i]));
        if (n[i] < 1 || n[i] > INT32_MAX - kOptChunk)
            return fail(o, MESHENV_E_ARG, at + std::to_string((long long)n[i]) + " elements");
        if (block[i] < 0 || block[i] >= kOptBlocks) return fail(o, MESHENV_E_ARG, at + "block " + std::to_string(block[i]));
        // RMSprop takes the gradient and square_avg (in exp_avg_sq_dev) and no first moment
        const bool adam = op[i] & kOptAdam, polyak = op[i] & kOptPolyak, steps = adam || op[i] == kOptRmsprop;
        if (!param_dev[i] || steps != (grad_dev[i] != nullptr) || adam != (exp_avg_dev[i] != nullptr) ||
            steps != (exp_avg_sq_dev[i] != nullptr) || polyak != (target_dev[i] != nullptr))
            return fail(o, MESHENV_E_ARG, at + "the pointers do not match op " + std::to_string(op[i]));
        const uintptr_t all = (uintptr_t)param_dev[i] | (uintptr_t)grad_dev[i] | (uintptr_t)exp_avg_dev[i] |
                              (uintptr_t)exp_avg_sq_dev[i] | (uintptr_t)target_dev[i];
        if (all & 3) return fail(o, MESHENV_E_ARG, at + "a pointer is not 4-byte aligned");
        if (vec[i] != 0 && (vec[i] != 1 || (all & 15)))
            return fail(o, MESHENV_E_ARG, at + "vec = " + std::to_string(vec[i]) + " on pointers that are not all 16-byte aligned");
        n_jobs += (n[i] + kOptChunk - 1) / kOptChunk;
    }
    if (n_jobs > INT32_MAX) return fail(o, MESHENV_E_ARG, "meshenv_optim_bind: more than 2^31 - 1 workgroups");
    const size_t jobs_at = ((size_t)n_seg * sizeof(OptSeg) + 15) / 16 * 16;
    const size_t bytes = jobs_at + (size_t)n_jobs * sizeof(OptJob);
    OptProgram &P = o->prog[program];
    DeviceGuard guard(o->device);
    if (guard.err != hipSuccess) return fail(o, MESHENV_E_HIP, "meshenv_optim_bind: hipSetDevice failed");
    // the staging block is free once its last upload is done; work on another stream may still read the tables
    if (o->used && o->last_stream != o->stream && hipStreamSynchronize(o->last_stream) != hipSuccess)
        return fail(o, MESHENV_E_HIP, "meshenv_optim_bind: hipStreamSynchronize failed");
    if (P.copied && hipEventSynchronize(P.copied) != hipSuccess)
        return fail(o, MESHENV_E_HIP, "meshenv_optim_bind: hipEventSynchronize failed");
    P.bound = false;
    if (bytes > P.cap) {
        if (o->used && hipStreamSynchronize(o->stream) != hipSuccess)     // a launch in flight reads the old tables
            return fail(o, MESHENV_E_HIP, "meshenv_optim_bind: hipStreamSynchronize failed");
        if (P.dev) (void)hipFree(P.dev);
        if (P.host) (void)hipHostFree(P.host);
        P.dev = P.host = nullptr;
        P.cap = 0;
        const size_t cap = bytes + bytes / 2;
        if (hipMalloc((void **)&P.dev, cap) != hipSuccess || hipHostMalloc((void **)&P.host, cap, hipHostMallocDefault) != hipSuccess ||
            (!P.copied && hipEventCreateWithFlags(&P.copied, hipEventDisableTiming) != hipSuccess))
            return fail(o, MESHENV_E_HIP, "meshenv_optim_bind: allocation failed");
        P.cap = cap;
    }
    OptSeg *segs = reinterpret_cast<OptSeg *>(P.host);
    OptJob *jobs = reinterpret_cast<OptJob *>(P.host + jobs_at);
    int j = 0;
    for (int i = 0; i < n_seg; i++) {
        segs[i] = OptSeg{param_dev[i], grad_dev[i], exp_avg_dev[i], exp_avg_sq_dev[i], target_dev[i], (int32_t)n[i], op[i], block[i], vec[i]};
        for (int64_t first = 0; first < n[i]; first += kOptChunk) jobs[j++] = OptJob{i, (int32_t)first};
    }
    if (hipMemcpyAsync(P.dev, P.host, bytes, hipMemcpyHostToDevice, o->stream) != hipSuccess ||
        hipEventRecord(P.copied, o->stream) != hipSuccess)
        return fail(o, MESHENV_E_HIP, "meshenv_optim_bind: upload failed");
    o->last_stream = P.ordered = o->stream;
    o->used = true;
    P.jobs_at = jobs_at;
    P.n_jobs = (int)n_jobs;
    P.n_seg = n_seg;
    P.bound = true;
    return MESHENV_OK;
}

int meshenv_optim_step(MeshOptim *o, int program, const MeshOptimScalars *scalars)
{
    return optim_step_launch(o, program, scalars, nullptr, "meshenv_optim_step");
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ the on-policy rollout buffer
static_assert(MESHENV_ROLLOUT_CHUNK == kRgChunk && MESHENV_ROLLOUT_FIELDS == 2 + kRgScalars, "include/meshenv_rollout.h and csrc/meshenv_rollout.h disagree");
static_assert((long long)MESHENV_ROLLOUT_MAX_ROWS * kRgObs + kRgChunk <= INT32_MAX, "k_rollout_gather indexes in int32");

struct MeshRolloutBuffer : HandleBase {};

extern "C" {

int meshenv_rollout_create(int device, void *stream, MeshRolloutBuffer **out)
{
    return create_handle("meshenv_rollout_create", device, stream, out);
}

void meshenv_rollout_destroy(MeshRolloutBuffer *r) { destroy_handle(r, nullptr); }

const char *meshenv_rollout_last_error(const MeshRolloutBuffer *r) { return last_error(r); }

int meshenv_rollout_set_stream(MeshRolloutBuffer *r, void *stream) { return set_stream(r, stream); }

int meshenv_rollout_gather(MeshRolloutBuffer *r, int T, int n_envs, const void *perm_dev, int perm_bytes,
                           const float *const *in_dev, float *const *out_dev, int variant)
{
    if (!r) return MESHENV_E_ARG;
    const char *fn = "meshenv_rollout_gather";
    if (T < 1 || n_envs < 1 || (long long)T * n_envs > MESHENV_ROLLOUT_MAX_ROWS)
        return fail(r, MESHENV_E_ARG, std::string(fn) + ": T >= 1, n_envs >= 1 and T * n_envs <= 2^24 - 16 are required");
    if (perm_bytes != 4 && perm_bytes != 8) return fail(r, MESHENV_E_ARG, std::string(fn) + ": perm_bytes is 4 (int32) or 8 (int64)");
    if (variant != 0 && variant != 1) return fail(r, MESHENV_E_ARG, std::string(fn) + ": variant is 0 or 1");
    if (!perm_dev || !in_dev || !out_dev) return fail(r, MESHENV_E_ARG, std::string(fn) + ": perm_dev, in_dev and out_dev are required");
    if ((uintptr_t)perm_dev & (uintptr_t)(perm_bytes - 1)) return fail(r, MESHENV_E_ARG, std::string(fn) + ": perm_dev is off the alignment of its indices");
    const int rows = T * n_envs;
    const size_t width[MESHENV_ROLLOUT_FIELDS] = {kRgObs, kRgAct, 1, 1, 1, 1};
    for (int f = 0; f < MESHENV_ROLLOUT_FIELDS; f++) {
        if (!in_dev[f] || !out_dev[f]) return fail(r, MESHENV_E_ARG, std::string(fn) + ": null pointer for field " + std::to_string(f));
        if (((uintptr_t)in_dev[f] | (uintptr_t)out_dev[f]) & 3)
            return fail(r, MESHENV_E_ARG, std::string(fn) + ": a pointer of field " + std::to_string(f) + " is not 4-byte aligned");
    }
    // every output against every input and every other output: a thread reads rows that other threads write
    for (int f = 0; f < MESHENV_ROLLOUT_FIELDS; f++) {
        const uintptr_t o0 = (uintptr_t)out_dev[f], o1 = o0 + width[f] * rows * sizeof(float);
        for (int k = 0; k < MESHENV_ROLLOUT_FIELDS; k++) {
            const uintptr_t i0 = (uintptr_t)in_dev[k], i1 = i0 + width[k] * rows * sizeof(float);
            const uintptr_t p0 = (uintptr_t)out_dev[k], p1 = p0 + width[k] * rows * sizeof(float);
            if ((o0 < i1 && i0 < o1) || (k != f && o0 < p1 && p0 < o1))
                return fail(r, MESHENV_E_ARG, std::string(fn) + ": the output of field " + std::to_string(f) + " overlaps field " + std::to_string(k));
        }
        const uintptr_t q0 = (uintptr_t)perm_dev, q1 = q0 + (size_t)perm_bytes * rows;
        if (o0 < q1 && q0 < o1) return fail(r, MESHENV_E_ARG, std::string(fn) + ": the output of field " + std::to_string(f) + " overlaps perm_dev");
    }
    if (variant == 1 && (((uintptr_t)in_dev[0] | (uintptr_t)out_dev[0]) & 7))
        return fail(r, MESHENV_E_ARG, std::string(fn) + ": variant 1 needs both observation pointers 8-byte aligned");
    RolloutGatherArgs A{};
    A.obs = in_dev[0]; A.act = in_dev[1]; A.obs_out = out_dev[0]; A.act_out = out_dev[1];
    for (int f = 0; f < kRgScalars; f++) { A.scalar[f] = in_dev[2 + f]; A.scalar_out[f] = out_dev[2 + f]; }
    A.perm = perm_dev; A.perm64 = perm_bytes == 8;
    A.T = T; A.n = n_envs; A.rows = rows;
    A.obs_blocks = (rows * kRgObs + kRgChunk - 1) / kRgChunk;
    A.act_blocks = (rows * kRgAct + kRgChunk - 1) / kRgChunk;
    A.scalar_blocks = (rows + kRgChunk - 1) / kRgChunk;
    const int grid = A.obs_blocks + A.act_blocks + kRgScalars * A.scalar_blocks;
    DeviceGuard guard(r->device);
    return launch(r, guard, fn, [&] {
        if (variant == 1) hipLaunchKernelGGL(k_rollout_gather<true>, dim3(grid), dim3(kRgThreads), 0, r->stream, A);
        else hipLaunchKernelGGL(k_rollout_gather<false>, dim3(grid), dim3(kRgThreads), 0, r->stream, A);
    });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ PPO.train / A2C.train in one call
static_assert(MESHENV_TRAIN_OUTPUTS == kTrOut, "include/meshenv_onpolicy_train.h and csrc/meshenv_onpolicy_train.h disagree");

struct MeshOnPolicyTrain : HandleBase {
    float *buf = nullptr;       // the tally (kTlWords doubles, padded to 16), stop[K_max + 1] (padded), the kPgOut outputs of K_max minibatches
};

namespace {

constexpr size_t kTrTallyFloats = 32, kTrStopFloats = MESHENV_TRAIN_MAX_MINIBATCHES + 16;
static_assert(kTlWords * 2 <= kTrTallyFloats, "the tally fits its block");

}  // namespace

extern "C" {

int meshenv_onpolicy_train_create(int device, void *stream, MeshOnPolicyTrain **out)
{
    const int rc = create_handle("meshenv_onpolicy_train_create", device, stream, out);
    if (rc != MESHENV_OK) return rc;
    MeshOnPolicyTrain *t = *out;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess ||
        !zeroed_once(t, &t->buf, kTrTallyFloats + kTrStopFloats + (size_t)MESHENV_TRAIN_MAX_MINIBATCHES * kPgOut)) {
        g_create_error = "meshenv_onpolicy_train_create: allocation failed";
        if (t->buf) (void)hipFree(t->buf);
        delete t;
        *out = nullptr;
        return MESHENV_E_HIP;
    }
    return MESHENV_OK;
}

void meshenv_onpolicy_train_destroy(MeshOnPolicyTrain *t) { destroy_handle(t, t ? t->buf : nullptr); }

const char *meshenv_onpolicy_train_last_error(const MeshOnPolicyTrain *t) { return last_error(t); }

int meshenv_onpolicy_train_set_stream(MeshOnPolicyTrain *t, void *stream) { return set_stream(t, stream); }

}  // extern "C"

// ------------------------------------------------------------------------------------------ the counted train() of learn()
static_assert(MESHENV_LEARN_MAX_ENTRIES == 1 << 20, "include/meshenv_onpolicy_learn.h");

struct MeshOnPolicyLearn : HandleBase {
    char *table = nullptr;         // [entries][blocks][2] doubles on the device
    char *host = nullptr;          // pinned staging of the same layout
    size_t cap = 0;                // bytes of both
    hipEvent_t copied = nullptr;   // the last upload from `host`
    hipStream_t ordered = nullptr; // the stream that is known to be ordered after that upload and the zeroing of the words
    int32_t *words = nullptr;      // the caller's: MESHENV_LEARN_WORDS words, then count[1 ..]
    int64_t n_words = 0;
    int entries = 0, blocks = 0;
    int64_t claimed = 0;           // entries that the runs since the bind may reach: the sum of their K
    bool used = false, bound = false;
};

namespace {

// What meshenv_onpolicy_learn_run adds to a train(): the handle, the scalars, the history row.
struct CountedRun {
    MeshOnPolicyLearn *l;
    const MeshOptimCounted *hyper;
    double *row;
};

// The refusals of a counted run that need K, and the claim of its K entries: before anything is enqueued.
int counted_claim(MeshOnPolicyTrain *t, const std::string &fn, const CountedRun &c, const MeshOptim *o, int program, long long K)
{
    MeshOnPolicyLearn *l = c.l;
    if (l->claimed + K > l->entries)
        return fail(t, MESHENV_E_ARG, fn + ": " + std::to_string(K) + " minibatches after " + std::to_string((long long)l->claimed) +
                       " claimed since the bind; the table has " + std::to_string(l->entries) + " entries");
    if (l->n_words < MESHENV_LEARN_WORDS + K)
        return fail(t, MESHENV_E_ARG, fn + ": the bound words hold fewer than " + std::to_string(MESHENV_LEARN_WORDS + K));
    const OptProgram &P = o->prog[program];
    const OptSeg *segs = reinterpret_cast<const OptSeg *>(P.host);
    for (int i = 0; i < P.n_seg; i++) {
        if (segs[i].block >= l->blocks) return fail(t, MESHENV_E_ARG, fn + ": the program reads a block that the table does not have");
        if (!std::isfinite(c.hyper->lr[segs[i].block])) return fail(t, MESHENV_E_ARG, fn + ": lr is not finite");
    }
    if (l->ordered != t->stream) {           // the table was uploaded on another stream: order this one after the upload
        DeviceGuard guard(t->device);
        if (guard.err != hipSuccess || hipStreamWaitEvent(t->stream, l->copied, 0) != hipSuccess)
            return fail(t, MESHENV_E_HIP, fn + ": hipStreamWaitEvent failed");
        l->ordered = t->stream;
    }
    l->claimed += K;
    l->used = true;
    return MESHENV_OK;
}

// The body of meshenv_onpolicy_train_run (counted: NULL) and of meshenv_onpolicy_learn_run under the name `fn`.
int onpolicy_train_enqueue(const std::string &fn, MeshOnPolicyTrain *t, MeshPpoGrad *g, MeshOptim *o, int program,
                           MeshRolloutBuffer *r, MeshPolicy *policy, int T, int n_envs, const float *const *in_dev,
                           float *const *gather_dev, const void *perm_dev, int perm_bytes, int n_epochs, int batch_size, int a2c,
                           double clip_range, float ent_coef, float vf_coef, int normalize_advantage, int clip_grad,
                           float max_grad_norm, double target_kl, const MeshOptimScalars *scalars, int n_scalars, double *out_dev,
                           const CountedRun *counted)
{
    if (!g || !o || !r) return fail(t, MESHENV_E_ARG, fn + ": the gradient, optimiser and rollout-buffer handles are required");
    if (g->device != t->device || o->device != t->device || r->device != t->device || (policy && policy->device != t->device))
        return fail(t, MESHENV_E_ARG, fn + ": the handles are on different devices");
    if (!g->bound) return fail(t, MESHENV_E_STATE, fn + ": the gradient handle has no tensors bound (meshenv_ppo_grad_bind)");
    if (program < 0 || program >= MESHENV_OPTIM_PROGRAMS) return fail(t, MESHENV_E_ARG, fn + ": program out of range");
    if (!o->prog[program].bound) return fail(t, MESHENV_E_STATE, fn + ": the optimiser's program is not bound (meshenv_optim_bind)");
    if (policy && (!policy->loaded || !policy->live))
        return fail(t, MESHENV_E_STATE, fn + ": the policy has no tensors bound (meshenv_policy_bind)");
    if (g->stream != t->stream || o->stream != t->stream || r->stream != t->stream || (policy && policy->stream != t->stream))
        return fail(t, MESHENV_E_STATE, fn + ": the handles are on different streams (set_stream them to one)");
    if (n_epochs < 1 || batch_size < 1) return fail(t, MESHENV_E_ARG, fn + ": n_epochs >= 1 and batch_size >= 1 are required");
    if (!(target_kl >= 0.0)) return fail(t, MESHENV_E_ARG, fn + ": target_kl must be >= 0 (+inf: none), not negative or NaN");
    if (T < 1 || n_envs < 1 || (long long)T * n_envs > MESHENV_ROLLOUT_MAX_ROWS)
        return fail(t, MESHENV_E_ARG, fn + ": T >= 1, n_envs >= 1 and T * n_envs <= 2^24 - 16 are required");
    if (!in_dev || !gather_dev || !perm_dev || (!scalars && !counted) || !out_dev || ((uintptr_t)out_dev & 7))
        return fail(t, MESHENV_E_ARG, fn + ": in_dev, gather_dev, perm_dev, scalars and an 8-byte aligned out_dev are required");
    if (perm_bytes != 4 && perm_bytes != 8) return fail(t, MESHENV_E_ARG, fn + ": perm_bytes is 4 (int32) or 8 (int64)");
    const int rows = T * n_envs;
    const int per_epoch = (rows + batch_size - 1) / batch_size;
    const long long K = (long long)n_epochs * per_epoch;
    if (K > MESHENV_TRAIN_MAX_MINIBATCHES)
        return fail(t, MESHENV_E_ARG, fn + ": " + std::to_string(K) + " minibatches; at most " + std::to_string(MESHENV_TRAIN_MAX_MINIBATCHES));
    if (!counted && n_scalars != K)
        return fail(t, MESHENV_E_ARG, fn + ": " + std::to_string(n_scalars) + " scalar sets for " + std::to_string(K) + " minibatches");
    for (int f = 0; f < MESHENV_ROLLOUT_FIELDS; f++)
        if (!in_dev[f] || !gather_dev[f]) return fail(t, MESHENV_E_ARG, fn + ": null pointer for field " + std::to_string(f));
    OptCounted C{};
    if (counted) {
        const int rc = counted_claim(t, fn, *counted, o, program, K);
        if (rc != MESHENV_OK) return rc;
        const MeshOnPolicyLearn *l = counted->l;
        const MeshOptimCounted &h = *counted->hyper;
        C.table = reinterpret_cast<const double *>(l->table);
        C.error = l->words + MESHENV_LEARN_WORD_ERROR;
        C.entries = l->entries; C.blocks = l->blocks;
        for (int b = 0; b < kOptBlocks; b++) { C.lr[b] = h.lr[b]; C.w1[b] = h.w1[b]; C.beta2[b] = h.beta2[b]; C.w2[b] = h.w2[b]; C.eps[b] = h.eps[b]; }
        C.tau = h.tau; C.one_minus_tau = h.one_minus_tau;
    }
    int32_t *count = counted ? counted->l->words + MESHENV_LEARN_WORD_STEPS : nullptr;   // count[0] is the step word
    double *tally = reinterpret_cast<double *>(t->buf);
    int32_t *stop = reinterpret_cast<int32_t *>(t->buf + kTrTallyFloats);
    float *pg_out = t->buf + kTrTallyFloats + kTrStopFloats;
    const float *obs = gather_dev[0], *act = gather_dev[1], *old = gather_dev[3], *adv = gather_dev[4], *ret = gather_dev[5];
    int m = 0;
    for (int e = 0; e < n_epochs; e++) {
        const char *perm = (const char *)perm_dev + (size_t)e * rows * perm_bytes;
        int rc = meshenv_rollout_gather(r, T, n_envs, perm, perm_bytes, in_dev, gather_dev, 0);
        if (rc != MESHENV_OK) return fail(t, rc, fn + ": " + r->err);
        for (int k = 0; k < per_epoch; k++, m++) {
            const int a = k * batch_size, n = rows - a < batch_size ? rows - a : batch_size;
            float *out_m = pg_out + (size_t)m * kPgOut;
            rc = meshenv_ppo_grad_backward(g, n, obs + (size_t)a * kRgObs, act + (size_t)a * kRgAct, a2c ? nullptr : old + a, adv + a, ret + a,
                                           a2c, clip_range, ent_coef, vf_coef, normalize_advantage, clip_grad, max_grad_norm, out_m,
                                           nullptr, nullptr);
            if (rc != MESHENV_OK) return fail(t, rc, fn + ": " + g->err);
            TrainGate G{};
            G.stop = stop + m; G.pg_out = out_m; G.tally = tally; G.kl_limit = 1.5 * target_kl;
            G.first_of_epoch = k == 0; G.first_of_train = m == 0;
            if (counted) {
                C.count = count + m;
                rc = optim_step_launch(o, program, nullptr, &G, fn.c_str(), nullptr, &C);
            } else {
                rc = optim_step_launch(o, program, scalars + m, &G, fn.c_str());
            }
            if (rc != MESHENV_OK) return fail(t, rc, fn + ": " + o->err);
        }
    }
    DeviceGuard guard(t->device);
    int rc = launch(t, guard, fn.c_str(), [&] {
        if (counted)
            hipLaunchKernelGGL(k_learn_finish, dim3(1), dim3(kTrFinishThreads), 0, t->stream, in_dev[2], in_dev[5], rows, g->log_std,
                               (const double *)tally, out_dev, count, (int)K, counted->l->words + MESHENV_LEARN_WORD_N_UPDATES);
        else
            hipLaunchKernelGGL(k_train_finish, dim3(1), dim3(kTrFinishThreads), 0, t->stream, in_dev[2], in_dev[5], rows, g->log_std,
                               (const double *)tally, out_dev);
    }, "finish launch");
    if (rc != MESHENV_OK || !policy) return rc;
    rc = meshenv_policy_refresh(policy);
    return rc == MESHENV_OK ? rc : fail(t, rc, fn + ": " + policy->err);
}

}  // namespace

extern "C" {

int meshenv_onpolicy_train_run(MeshOnPolicyTrain *t, MeshPpoGrad *g, MeshOptim *o, int program, MeshRolloutBuffer *r,
                               MeshPolicy *policy, int T, int n_envs, const float *const *in_dev, float *const *gather_dev,
                               const void *perm_dev, int perm_bytes, int n_epochs, int batch_size, int a2c, double clip_range,
                               float ent_coef, float vf_coef, int normalize_advantage, int clip_grad, float max_grad_norm,
                               double target_kl, const MeshOptimScalars *scalars, int n_scalars, double *out_dev)
{
    if (!t) return MESHENV_E_ARG;
    return onpolicy_train_enqueue("meshenv_onpolicy_train_run", t, g, o, program, r, policy, T, n_envs, in_dev, gather_dev, perm_dev,
                                  perm_bytes, n_epochs, batch_size, a2c, clip_range, ent_coef, vf_coef, normalize_advantage, clip_grad,
                                  max_grad_norm, target_kl, scalars, n_scalars, out_dev, nullptr);
}

int meshenv_onpolicy_learn_create(int device, void *stream, MeshOnPolicyLearn **out)
{
    return create_handle("meshenv_onpolicy_learn_create", device, stream, out);
}

void meshenv_onpolicy_learn_destroy(MeshOnPolicyLearn *l)
{
    if (!l) return;
    DeviceGuard guard(l->device);
    (void)hipStreamSynchronize(l->stream);
    if (l->copied) {
        (void)hipEventSynchronize(l->copied);
        (void)hipEventDestroy(l->copied);
    }
    if (l->table) (void)hipFree(l->table);
    if (l->host) (void)hipHostFree(l->host);
    delete l;
}

const char *meshenv_onpolicy_learn_last_error(const MeshOnPolicyLearn *l) { return last_error(l); }

int meshenv_onpolicy_learn_set_stream(MeshOnPolicyLearn *l, void *stream) { return set_stream(l, stream); }

int meshenv_onpolicy_learn_bind(MeshOnPolicyLearn *l, const double *table_host, int entries, int blocks, int32_t *words_dev,
                                int64_t n_words)
{
    if (!l) return MESHENV_E_ARG;
    const std::string fn = "meshenv_onpolicy_learn_bind";
    if (!table_host || !words_dev || ((uintptr_t)words_dev & 3))
        return fail(l, MESHENV_E_ARG, fn + ": table_host and a 4-byte aligned words_dev are required");
    if (entries < 1 || entries > MESHENV_LEARN_MAX_ENTRIES)
        return fail(l, MESHENV_E_ARG, fn + ": " + std::to_string(entries) + " entries; 1 .. " + std::to_string(MESHENV_LEARN_MAX_ENTRIES));
    if (blocks < 1 || blocks > MESHENV_OPTIM_BLOCKS) return fail(l, MESHENV_E_ARG, fn + ": blocks is 1 .. " + std::to_string(MESHENV_OPTIM_BLOCKS));
    if (n_words < MESHENV_LEARN_WORDS + 1)
        return fail(l, MESHENV_E_ARG, fn + ": words_dev holds the " + std::to_string(MESHENV_LEARN_WORDS) + " words and count[1 ..] of a train()");
    const size_t doubles = (size_t)entries * blocks * 2, bytes = doubles * sizeof(double);
    for (size_t i = 0; i < doubles; i++)
        if (!std::isfinite(table_host[i]) || (i % 2 == 0 && table_host[i] == 0.0))
            return fail(l, MESHENV_E_ARG, fn + ": entry " + std::to_string(i / 2 / blocks) + " is not finite or has bias_correction1 = 0");
    DeviceGuard guard(l->device);
    if (guard.err != hipSuccess) return fail(l, MESHENV_E_HIP, fn + ": hipSetDevice failed");
    // the staging block is free once its last upload is done
    if (l->copied && hipEventSynchronize(l->copied) != hipSuccess) return fail(l, MESHENV_E_HIP, fn + ": hipEventSynchronize failed");
    l->bound = false;
    if (bytes > l->cap) {
        // a launch in flight reads the old table
        if (l->used && hipStreamSynchronize(l->ordered) != hipSuccess)
            return fail(l, MESHENV_E_HIP, fn + ": hipStreamSynchronize failed");
        if (l->table) (void)hipFree(l->table);
        if (l->host) (void)hipHostFree(l->host);
        l->table = l->host = nullptr;
        l->cap = 0;
        if (hipMalloc((void **)&l->table, bytes) != hipSuccess || hipHostMalloc((void **)&l->host, bytes, hipHostMallocDefault) != hipSuccess ||
            (!l->copied && hipEventCreateWithFlags(&l->copied, hipEventDisableTiming) != hipSuccess))
            return fail(l, MESHENV_E_HIP, fn + ": allocation failed");
        l->cap = bytes;
    }
    std::memcpy(l->host, table_host, bytes);
    if (hipMemcpyAsync(l->table, l->host, bytes, hipMemcpyHostToDevice, l->stream) != hipSuccess ||
        hipMemsetAsync(words_dev, 0, MESHENV_LEARN_WORDS * sizeof(int32_t), l->stream) != hipSuccess ||
        hipEventRecord(l->copied, l->stream) != hipSuccess)
        return fail(l, MESHENV_E_HIP, fn + ": upload failed");
    l->ordered = l->stream;
    l->words = words_dev;
    l->n_words = n_words;
    l->entries = entries;
    l->blocks = blocks;
    l->claimed = 0;
    l->bound = true;
    return MESHENV_OK;
}

int meshenv_onpolicy_learn_run(MeshOnPolicyLearn *l, MeshOnPolicyTrain *t, MeshPpoGrad *g, MeshOptim *o, int program,
                               MeshRolloutBuffer *r, MeshPolicy *policy, int T, int n_envs, const float *const *in_dev,
                               float *const *gather_dev, const void *perm_dev, int perm_bytes, int n_epochs, int batch_size, int a2c,
                               double clip_range, float ent_coef, float vf_coef, int normalize_advantage, int clip_grad,
                               float max_grad_norm, double target_kl, const MeshOptimCounted *counted, double *history_dev,
                               int iteration, int iterations)
{
    if (!l) return MESHENV_E_ARG;
    const std::string fn = "meshenv_onpolicy_learn_run";
    if (!t) return fail(l, MESHENV_E_ARG, fn + ": the train handle is required");
    if (!counted || !history_dev || ((uintptr_t)history_dev & 7))
        return fail(l, MESHENV_E_ARG, fn + ": counted and an 8-byte aligned history_dev are required");
    if (iterations < 1 || iteration < 0 || iteration >= iterations)
        return fail(l, MESHENV_E_ARG, fn + ": iteration " + std::to_string(iteration) + " is outside [0, " + std::to_string(iterations) + ")");
    if (!l->bound) return fail(l, MESHENV_E_STATE, fn + ": no table bound (meshenv_onpolicy_learn_bind)");
    if (l->device != t->device) return fail(l, MESHENV_E_ARG, fn + ": the handles are on different devices");
    if (l->stream != t->stream) return fail(l, MESHENV_E_STATE, fn + ": the handles are on different streams (set_stream them to one)");
    const CountedRun run{l, counted, history_dev + (size_t)iteration * MESHENV_TRAIN_OUTPUTS};
    const int rc = onpolicy_train_enqueue(fn, t, g, o, program, r, policy, T, n_envs, in_dev, gather_dev, perm_dev, perm_bytes, n_epochs,
                                          batch_size, a2c, clip_range, ent_coef, vf_coef, normalize_advantage, clip_grad, max_grad_norm,
                                          target_kl, nullptr, 0, run.row, &run);
    return rc == MESHENV_OK ? rc : fail(l, rc, t->err);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ SAC.train / TD3.train in one call
static_assert(MESHENV_OFFTRAIN_OUTPUTS == kOffOut, "include/meshenv_offpolicy_train.h and csrc/meshenv_offpolicy_train.h disagree");
static_assert(MESHENV_OFFTRAIN_SAMPLE_FLOATS == 2 * kObsDim + 3 + 2, "the sample workspace holds the five fields");

struct MeshOffPolicyTrain : HandleBase {
    float *slots = nullptr;     // [MESHENV_OFFTRAIN_MAX_STEPS][kOffSlot]: critic_loss actor_loss ent_coef_loss ent_coef per step
};

extern "C" {

int meshenv_offpolicy_train_create(int device, void *stream, MeshOffPolicyTrain **out)
{
    const int rc = create_handle("meshenv_offpolicy_train_create", device, stream, out);
    if (rc != MESHENV_OK) return rc;
    MeshOffPolicyTrain *t = *out;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess || !zeroed_once(t, &t->slots, (size_t)MESHENV_OFFTRAIN_MAX_STEPS * kOffSlot)) {
        g_create_error = "meshenv_offpolicy_train_create: allocation failed";
        if (t->slots) (void)hipFree(t->slots);
        delete t;
        *out = nullptr;
        return MESHENV_E_HIP;
    }
    return MESHENV_OK;
}

void meshenv_offpolicy_train_destroy(MeshOffPolicyTrain *t) { destroy_handle(t, t ? t->slots : nullptr); }

const char *meshenv_offpolicy_train_last_error(const MeshOffPolicyTrain *t) { return last_error(t); }

int meshenv_offpolicy_train_set_stream(MeshOffPolicyTrain *t, void *stream) { return set_stream(t, stream); }

int meshenv_offpolicy_train_run(MeshOffPolicyTrain *t, MeshEnv *env, MeshTarget *target, MeshCriticGrad *cg, MeshActorGrad *sac_ag,
                                MeshTd3ActorGrad *td3_ag, MeshOptim *o, int critic_program, const float *store_dev, int rows, int size,
                                int batch, int K, uint64_t seed, uint64_t counter0, float *const *sample_dev, int chunk,
                                float *target_dev, const int32_t *actor_program, const MeshOptimScalars *critic_scalars,
                                const MeshOptimScalars *actor_scalars, int n_actor_scalars, double *out_dev)
{
    if (!t) return MESHENV_E_ARG;
    const std::string fn = "meshenv_offpolicy_train_run";
    if (!env || !target || !cg || !o) return fail(t, MESHENV_E_ARG, fn + ": the env, target, critic-gradient and optimiser handles are required");
    if ((sac_ag != nullptr) == (td3_ag != nullptr))
        return fail(t, MESHENV_E_ARG, fn + ": exactly one of the SAC and the TD3 actor-gradient handle is required");
    const bool sac = sac_ag != nullptr;
    const int ag_device = sac ? sac_ag->device : td3_ag->device;
    const hipStream_t ag_stream = sac ? sac_ag->stream : td3_ag->stream;
    if (env->device != t->device || target->device != t->device || cg->device != t->device || o->device != t->device || ag_device != t->device)
        return fail(t, MESHENV_E_ARG, fn + ": the handles are on different devices");
    const int kind = sac ? kTargetSAC : kTargetTD3;
    if (target->kind != kind || cg->kind != kind)
        return fail(t, MESHENV_E_ARG, fn + ": the target and critic-gradient handles are not of the actor-gradient handle's kind");
    if (!target->bound) return fail(t, MESHENV_E_STATE, fn + ": the target handle has no tensors bound (meshenv_target_bind)");
    if (!target->packed) return fail(t, MESHENV_E_STATE, fn + ": the target handle was never refreshed (meshenv_target_refresh)");
    if (!cg->bound) return fail(t, MESHENV_E_STATE, fn + ": the critic-gradient handle has no tensors bound (meshenv_critic_grad_bind)");
    if (!(sac ? sac_ag->bound : td3_ag->bound))
        return fail(t, MESHENV_E_STATE, fn + ": the actor-gradient handle has no tensors bound");
    if (K < 1 || K > MESHENV_OFFTRAIN_MAX_STEPS)
        return fail(t, MESHENV_E_ARG, fn + ": " + std::to_string(K) + " gradient steps; 1 to " + std::to_string(MESHENV_OFFTRAIN_MAX_STEPS) + " per call");
    if (batch < 1 || chunk < 1) return fail(t, MESHENV_E_ARG, fn + ": batch >= 1 and chunk >= 1 are required");
    if (!store_dev || !sample_dev || !target_dev || !actor_program || !critic_scalars || !out_dev || ((uintptr_t)out_dev & 7) ||
        ((uintptr_t)target_dev & 3))
        return fail(t, MESHENV_E_ARG, fn + ": store_dev, sample_dev, a 4-byte aligned target_dev, actor_program, critic_scalars and an "
                                           "8-byte aligned out_dev are required");
    for (int f = 0; f < 5; f++)
        if (!sample_dev[f]) return fail(t, MESHENV_E_ARG, fn + ": null sample buffer " + std::to_string(f));
    auto program_bound = [&](int p) { return p >= 0 && p < MESHENV_OPTIM_PROGRAMS && o->prog[p].bound; };
    if (critic_program < 0 || critic_program >= MESHENV_OPTIM_PROGRAMS) return fail(t, MESHENV_E_ARG, fn + ": critic program out of range");
    if (!program_bound(critic_program)) return fail(t, MESHENV_E_STATE, fn + ": the critic program is not bound (meshenv_optim_bind)");
    // the actor steps: k = phase, phase + period, ... and nothing else
    int n_actor = 0, polyak_updates = 0, phase = K, period = 1, last = -1;
    for (int k = 0; k < K; k++) {
        const int p = actor_program[k];
        if (p < 0) continue;
        if (p >= MESHENV_OPTIM_PROGRAMS) return fail(t, MESHENV_E_ARG, fn + ": actor program out of range at step " + std::to_string(k));
        if (!o->prog[p].bound)
            return fail(t, MESHENV_E_STATE, fn + ": program " + std::to_string(p) + " of step " + std::to_string(k) + " is not bound (meshenv_optim_bind)");
        if (n_actor == 0) phase = k;
        else if (n_actor == 1) period = k - last;
        else if (k - last != period) return fail(t, MESHENV_E_ARG, fn + ": the actor steps do not recur with one period");
        last = k;
        n_actor++;
        const OptSeg *segs = reinterpret_cast<const OptSeg *>(o->prog[p].host);
        bool polyak = false;
        for (int i = 0; i < o->prog[p].n_seg; i++) polyak = polyak || (segs[i].op & kOptPolyak) != 0;
        polyak_updates += polyak ? 1 : 0;
    }
    if (n_actor == 1) period = K;        // one actor step: any period that reaches past the call
    if (n_actor >= 2 && last + period < K) return fail(t, MESHENV_E_ARG, fn + ": the actor steps do not recur with one period");
    if (n_actor != n_actor_scalars || (n_actor > 0 && !actor_scalars))
        return fail(t, MESHENV_E_ARG, fn + ": " + std::to_string(n_actor_scalars) + " actor scalar sets for " + std::to_string(n_actor) + " actor steps");
    if (env->stream != t->stream || target->stream != t->stream || cg->stream != t->stream || o->stream != t->stream || ag_stream != t->stream)
        return fail(t, MESHENV_E_STATE, fn + ": the handles are on different streams (set_stream them to one)");
    if (chunk > K) chunk = K;
    if ((long long)chunk * batch > MESHENV_REPLAY_BATCHES_MAX_SAMPLES)
        return fail(t, MESHENV_E_ARG, fn + ": chunk * batch exceeds MESHENV_REPLAY_BATCHES_MAX_SAMPLES (2^24)");
    {   // the target buffer is written while the step's samples are still read
        const size_t width[5] = {kObsDim, 3, kObsDim, 1, 1};
        const uintptr_t y0 = (uintptr_t)target_dev, y1 = y0 + (size_t)batch * sizeof(float);
        for (int f = 0; f < 5; f++) {
            const uintptr_t s0 = (uintptr_t)sample_dev[f], s1 = s0 + (size_t)chunk * batch * width[f] * sizeof(float);
            if (y0 < s1 && s0 < y1) return fail(t, MESHENV_E_ARG, fn + ": target_dev overlaps sample buffer " + std::to_string(f));
        }
    }
    const bool learned = sac && sac_ag->log_ent_coef != nullptr;
    if (learned && optim_program_writes(o, critic_program, sac_ag->log_ent_coef) >= 0)
        return fail(t, MESHENV_E_ARG, fn + ": segment " + std::to_string(optim_program_writes(o, critic_program, sac_ag->log_ent_coef)) +
                                           " of the critic program writes log_ent_coef, which the noted critic step reads");
    float *obs = sample_dev[0], *act = sample_dev[1], *next = sample_dev[2], *dones = sample_dev[3], *rew = sample_dev[4];
    int a = 0;
    for (int k = 0; k < K; k++) {
        const int j = k % chunk;
        if (j == 0) {
            const int nb = K - k < chunk ? K - k : chunk;
            const int rc = meshenv_replay_sample_batches(env, store_dev, rows, size, batch, nb, seed, counter0 + (uint64_t)k, obs, act, next,
                                                         dones, rew, nullptr, nullptr);
            if (rc != MESHENV_OK) return fail(t, rc, fn + ": " + env->err);
        }
        const size_t at = (size_t)j * batch;
        float *slot = t->slots + (size_t)k * kOffSlot;
        int rc = meshenv_target_forward(target, batch, next + at * kObsDim, rew + at, dones + at, nullptr, 1, seed, counter0 + (uint64_t)k,
                                        target_dev, nullptr, nullptr, nullptr, nullptr, nullptr);
        if (rc != MESHENV_OK) return fail(t, rc, fn + ": " + target->err);
        rc = meshenv_critic_grad_backward(cg, batch, obs + at * kObsDim, act + at * 3, target_dev, slot, nullptr, nullptr, nullptr, nullptr);
        if (rc != MESHENV_OK) return fail(t, rc, fn + ": " + cg->err);
        OptNote note{learned ? sac_ag->log_ent_coef : nullptr, slot + 3};
        rc = optim_step_launch(o, critic_program, critic_scalars + k, nullptr, "meshenv_offpolicy_train_run", learned ? &note : nullptr);
        if (rc != MESHENV_OK) return fail(t, rc, fn + ": " + o->err);
        const int p = actor_program[k];
        if (p >= 0) {
            if (sac) {
                rc = meshenv_actor_grad_backward(sac_ag, batch, obs + at * kObsDim, nullptr, 1, seed, counter0 + (uint64_t)k, slot + 1, nullptr,
                                                 nullptr, nullptr);
                if (rc != MESHENV_OK) return fail(t, rc, fn + ": " + sac_ag->err);
            } else {
                rc = meshenv_td3_actor_grad_backward(td3_ag, batch, obs + at * kObsDim, slot + 1, nullptr, nullptr);
                if (rc != MESHENV_OK) return fail(t, rc, fn + ": " + td3_ag->err);
            }
            rc = optim_step_launch(o, p, actor_scalars + a, nullptr, "meshenv_offpolicy_train_run");
            if (rc != MESHENV_OK) return fail(t, rc, fn + ": " + o->err);
            a++;
        }
        if (sac || p >= 0) {       // a tensor the target handle has bound changed: SAC's actor every step, TD3's targets on actor steps
            rc = meshenv_target_refresh(target);
            if (rc != MESHENV_OK) return fail(t, rc, fn + ": " + target->err);
        }
    }
    OffFinishArgs A{};
    A.slots = t->slots; A.out = out_dev; A.K = K; A.phase = phase; A.period = period;
    A.actor_steps = n_actor; A.polyak_updates = polyak_updates;
    A.mode = !sac ? kOffTd3 : learned ? kOffSacLearned : kOffSacFixed;
    A.ent_coef = sac ? sac_ag->ent_coef : 0.0f;
    DeviceGuard guard(t->device);
    return launch(t, guard, "meshenv_offpolicy_train_run", [&] {
        hipLaunchKernelGGL(k_offpolicy_finish, dim3(1), dim3(kTrFinishThreads), 0, t->stream, A);
    }, "finish launch");
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ the off-policy learn loop
// (include/meshenv_offpolicy_learn.h, csrc/meshenv_learn.h)
static_assert(MESHENV_UNIFORM_PHILOX_TAG == kUniformPhiloxTag, "include/meshenv_offpolicy_learn.h and csrc/meshenv_learn.h disagree");

struct MeshEpisodeStats : HandleBase {};

extern "C" {

// ---- live weights into a loaded FusedActor (the SAC twin of meshenv_policy_bind / meshenv_policy_refresh)
int meshenv_actor_bind(MeshActor *a, const float *const *tensors_dev, int n)
{
    if (!a) return MESHENV_E_ARG;
    if (!a->loaded) return fail(a, MESHENV_E_STATE, "meshenv_actor_bind: no weights loaded (meshenv_actor_load lays the buffer out)");
    if (!tensors_dev || n != 10)
        return fail(a, MESHENV_E_ARG, "meshenv_actor_bind: the SAC actor takes 10 tensors (w1 b1 w2 b2 w3 b3 mu_w mu_b log_std_w log_std_b)");
    for (int i = 0; i < n; i++)
        if (!tensors_dev[i]) return fail(a, MESHENV_E_ARG, "meshenv_actor_bind: null tensor");
    a->n_copies = pack_table(actor_layout(), tensors_dev, n, a->buf, a->table);
    a->live = true;
    return MESHENV_OK;
}

int meshenv_actor_refresh(MeshActor *a)
{
    if (!a) return MESHENV_E_ARG;
    if (!a->loaded || !a->live) return fail(a, MESHENV_E_STATE, "meshenv_actor_refresh: no tensors bound (meshenv_actor_bind)");
    return pack_refresh(a, "meshenv_actor_refresh");
}

const char *meshenv_actor_last_error(const MeshActor *a) { return last_error(a); }

// ---- warm-up actions and the steps that take them
int meshenv_uniform_actions(MeshEnv *h, int T, uint64_t seed, uint64_t counter, const float *low_high_host, float *actions_dev,
                            float *buffer_actions_dev)
{
    if (!h) return MESHENV_E_ARG;
    if (T < 1 || !low_high_host || !actions_dev || !buffer_actions_dev)
        return fail_arg(h, "meshenv_uniform_actions: T >= 1, the six bounds and both outputs are required");
    UniformArgs A{};
    for (int k = 0; k < 3; k++) {
        A.low[k] = low_high_host[k]; A.high[k] = low_high_host[3 + k];
        if (!std::isfinite(A.low[k]) || !std::isfinite(A.high[k]) || !(A.high[k] > A.low[k]))
            return fail_arg(h, "meshenv_uniform_actions: the bounds must be finite with high > low");
    }
    A.T = T; A.n = h->n_envs; A.seed = seed; A.counter = counter; A.actions = actions_dev; A.buffer_actions = buffer_actions_dev;
    MESHENV_ON_DEVICE(h);
    const long long total = (long long)T * h->n_envs;
    const long long want = (total + 255) / 256;
    const int blocks = want < 4096 ? (int)want : 4096;   // the kernel strides over the rest
    hipLaunchKernelGGL(k_uniform_actions, dim3(blocks), dim3(256), 0, h->stream, A);
    HIP_TRY(h, hipGetLastError());
    return MESHENV_OK;
}

int meshenv_step_actions_multi(MeshEnv *h, int T, const float *actions_dev, float *obs_dev, double *reward_dev, uint8_t *done_dev,
                               uint8_t *complete_dev, float *terminal_obs_dev, int auto_reset)
{
    if (!h) return MESHENV_E_ARG;
    if (T < 1 || !actions_dev || !obs_dev || !reward_dev || !done_dev || !complete_dev)
        return fail_arg(h, "meshenv_step_actions_multi: T >= 1 and non-null actions, obs, reward, done and complete are required");
    const size_t n = (size_t)h->n_envs;
    for (int t = 0; t < T; t++) {
        const int rc = launch_step(h, 1, actions_dev + (size_t)t * n * 3, obs_dev + (size_t)(t + 1) * n * kObsDim, reward_dev + (size_t)t * n,
                                   done_dev + (size_t)t * n, complete_dev + (size_t)t * n,
                                   terminal_obs_dev ? terminal_obs_dev + (size_t)t * n * kObsDim : nullptr, auto_reset);
        if (rc != MESHENV_OK) return rc;
    }
    return MESHENV_OK;
}

// ---- episode statistics
int meshenv_episode_stats_create(int device, void *stream, MeshEpisodeStats **out)
{
    return create_handle("meshenv_episode_stats_create", device, stream, out);
}

void meshenv_episode_stats_destroy(MeshEpisodeStats *s) { destroy_handle(s, nullptr); }

const char *meshenv_episode_stats_last_error(const MeshEpisodeStats *s) { return last_error(s); }

int meshenv_episode_stats_set_stream(MeshEpisodeStats *s, void *stream) { return set_stream(s, stream); }

int meshenv_episode_stats_update(MeshEpisodeStats *s, int T, int n, int window, const double *reward_dev, const uint8_t *done_dev,
                                 const uint8_t *complete_dev, double *carry_return_dev, int32_t *carry_len_dev, double *ring_dev,
                                 uint64_t *count_dev, double *work_return_dev, int32_t *work_len_dev)
{
    if (!s) return MESHENV_E_ARG;
    if (T < 1 || n < 1 || window < 1 || (long long)T * n >= (1LL << 31))
        return fail(s, MESHENV_E_ARG, "meshenv_episode_stats_update: T, n, window >= 1 and T * n < 2^31 are required");
    if (!reward_dev || !done_dev || !complete_dev || !carry_return_dev || !carry_len_dev || !ring_dev || !count_dev || !work_return_dev ||
        !work_len_dev)
        return fail(s, MESHENV_E_ARG, "meshenv_episode_stats_update: null device pointer");
    if ((uintptr_t)count_dev % 8 != 0) return fail(s, MESHENV_E_ARG, "meshenv_episode_stats_update: count_dev must be 8-byte aligned");
    EpisodeArgs A{};
    A.T = T; A.n = n; A.W = window; A.reward = reward_dev; A.done = done_dev; A.complete = complete_dev;
    A.carry_return = carry_return_dev; A.carry_len = carry_len_dev; A.ring = ring_dev; A.count = (unsigned long long *)count_dev;
    A.work_return = work_return_dev; A.work_len = work_len_dev;
    DeviceGuard guard(s->device);
    return launch(s, guard, "meshenv_episode_stats_update", [&] {
        hipLaunchKernelGGL(k_episode_stats, dim3(1), dim3(kEpThreads), 0, s->stream, A);
    });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ the evaluation callback
// (include/meshenv_eval_callback.h, csrc/meshenv_eval_callback.h)
static_assert(MESHENV_EVAL_ROW_DOUBLES == kEvalRowDoubles && MESHENV_EVAL_STATE_DOUBLES == kEvalStateDoubles &&
              MESHENV_KEEP_BEST_MAX_ENTRIES == kKeepMaxEntries, "include/meshenv_eval_callback.h and csrc/meshenv_eval_callback.h disagree");
static_assert(sizeof(KeepTable) <= 2048, "the copy table travels as a kernel argument");

struct MeshEvalCallback : HandleBase {};

extern "C" {

// meshenv_evaluate's loop with eval_read_short and the pinned word taken out: what is enqueued depends on `steps` alone
int meshenv_evaluate_queued(MeshEnv *h, MeshPolicy *policy, MeshActor *actor, int sample, uint64_t seed, uint64_t counter, int steps,
                            const MeshEvalBuffers *bufs)
{
    if (!h) return MESHENV_E_ARG;
    if ((policy != nullptr) == (actor != nullptr)) return fail_arg(h, "meshenv_evaluate_queued: give exactly one of policy and actor");
    if (steps < 1) return fail_arg(h, "meshenv_evaluate_queued: steps must be >= 1");
    if (policy ? !policy->loaded : !actor->loaded) {
        h->err = "meshenv_evaluate_queued: the policy / actor has no weights loaded";
        return MESHENV_E_STATE;
    }
    if (policy ? (policy->device != h->device || policy->stream != h->stream) : (actor->device != h->device || actor->stream != h->stream)) {
        h->err = "meshenv_evaluate_queued: env and policy / actor must be on the same device and stream";
        return MESHENV_E_STATE;
    }
    EvalTallyArgs A;
    int rc = eval_check(h, "meshenv_evaluate_queued", bufs, &A);
    if (rc != MESHENV_OK) return rc;
    MESHENV_ON_DEVICE(h);
    const size_t n = (size_t)h->n_envs;
    // every allocation before the first launch: nothing is allocated on the per-step path
    if (!h->eval_act && (rc = dev_alloc(h, &h->eval_act, 2 * n * 3)) != MESHENV_OK) return rc;
    if (!bufs->obs_dev && !h->eval_obs) {
        if ((rc = dev_alloc(h, &h->eval_obs, n * kObsDim)) != MESHENV_OK || (rc = dev_alloc(h, &h->eval_reward, n)) != MESHENV_OK ||
            (rc = dev_alloc(h, &h->eval_done, n)) != MESHENV_OK || (rc = dev_alloc(h, &h->eval_complete, n)) != MESHENV_OK)
            return rc;
    }
    float *obs = bufs->obs_dev ? bufs->obs_dev : h->eval_obs;
    double *reward = bufs->obs_dev ? bufs->reward_dev : h->eval_reward;
    uint8_t *done = bufs->obs_dev ? bufs->done_dev : h->eval_done;
    uint8_t *complete = bufs->obs_dev ? bufs->complete_dev : h->eval_complete;
    float *act[2] = {h->eval_act, h->eval_act + n * 3};
    if ((rc = meshenv_reset(h, nullptr, obs)) != MESHENV_OK) return rc;
    if ((rc = eval_begin_launch(h, A)) != MESHENV_OK) return rc;
    if (actor && (rc = actor_launch(actor, "meshenv_evaluate_queued", (int)n, obs, nullptr, act[0], sample, seed, counter, nullptr)) != MESHENV_OK) {
        h->err = actor->err;
        return rc;
    }
    PolicyArgs P{};
    P.n = (int)n; P.obs = obs; P.sample = sample ? 1 : 0; P.seed = seed; P.actions = act[0];
    for (int t = 0; t < steps; t++) {
        if (policy) {
            P.counter = counter + (uint64_t)t;
            if ((rc = policy_launch(policy, "meshenv_evaluate_queued", P)) != MESHENV_OK) {
                h->err = policy->err;
                return rc;
            }
            rc = launch_step(h, 1, act[0], obs, reward, done, complete, nullptr, 1);
        } else {
            rc = meshenv_step_actor(h, actor, act[t & 1], obs, reward, done, complete, nullptr, 1, sample, seed, counter + (uint64_t)t + 1,
                                    act[(t + 1) & 1], nullptr);
        }
        if (rc != MESHENV_OK) return rc;
        if ((rc = eval_tally_launch(h, A, t, reward, done, complete)) != MESHENV_OK) return rc;
    }
    return MESHENV_OK;
}

int meshenv_eval_callback_create(int device, void *stream, MeshEvalCallback **out)
{
    return create_handle("meshenv_eval_callback_create", device, stream, out);
}

void meshenv_eval_callback_destroy(MeshEvalCallback *c) { destroy_handle(c, nullptr); }

const char *meshenv_eval_callback_last_error(const MeshEvalCallback *c) { return last_error(c); }

int meshenv_eval_callback_set_stream(MeshEvalCallback *c, void *stream) { return set_stream(c, stream); }

int meshenv_eval_reduce(MeshEvalCallback *c, int n_envs, int total, const MeshEvalBuffers *bufs, int row, int capacity,
                        double num_timesteps, double *history_dev, double *state_dev, int32_t *improved_dev)
{
    if (!c) return MESHENV_E_ARG;
    const std::string fn = "meshenv_eval_reduce";
    if (n_envs < 1 || total < 0 || capacity < 1 || row < 0 || row >= capacity)
        return fail(c, MESHENV_E_ARG, fn + ": n_envs >= 1, total >= 0 and 0 <= row < capacity are required");
    if (!bufs || bufs->struct_size != (int32_t)sizeof(MeshEvalBuffers))
        return fail(c, MESHENV_E_ARG, fn + ": MeshEvalBuffers missing or struct_size mismatch");
    if (!bufs->target_dev || !bufs->offset_dev || !bufs->count_dev || !bufs->ep_return_dev || !bufs->ep_length_dev || !bufs->ep_flags_dev ||
        !bufs->ep_n_elements_dev || !bufs->short_dev)
        return fail(c, MESHENV_E_ARG, fn + ": target, offset, count, ep_return, ep_length, ep_flags, ep_n_elements and short are required");
    if (!history_dev || !state_dev || !improved_dev || ((uintptr_t)history_dev & 7) || ((uintptr_t)state_dev & 7) || ((uintptr_t)improved_dev & 3))
        return fail(c, MESHENV_E_ARG, fn + ": 8-byte aligned history_dev and state_dev and a 4-byte aligned improved_dev are required");
    EvalReduceArgs A{};
    A.n = n_envs; A.total = total; A.row = row; A.num_timesteps = num_timesteps;
    A.target = bufs->target_dev; A.offset = bufs->offset_dev; A.count = bufs->count_dev;
    A.ep_return = bufs->ep_return_dev; A.ep_length = bufs->ep_length_dev; A.ep_flags = bufs->ep_flags_dev; A.ep_n_elem = bufs->ep_n_elements_dev;
    A.short_envs = bufs->short_dev; A.history = history_dev; A.state = state_dev; A.improved = improved_dev;
    DeviceGuard guard(c->device);
    return launch(c, guard, "meshenv_eval_reduce", [&] {
        hipLaunchKernelGGL(k_eval_reduce, dim3(1), dim3(64), 0, c->stream, A);
    });
}

int meshenv_keep_best(MeshEvalCallback *c, const MeshKeepEntry *entries_host, int n_entries, float *best_dev, int64_t best_floats,
                      const int32_t *improved_dev)
{
    if (!c) return MESHENV_E_ARG;
    const std::string fn = "meshenv_keep_best";
    if (!entries_host || n_entries < 1 || n_entries > kKeepMaxEntries)
        return fail(c, MESHENV_E_ARG, fn + ": 1 to " + std::to_string(kKeepMaxEntries) + " entries are required");
    if (!best_dev || !improved_dev || best_floats < 1 || ((uintptr_t)best_dev & 3) || ((uintptr_t)improved_dev & 3))
        return fail(c, MESHENV_E_ARG, fn + ": 4-byte aligned best_dev and improved_dev and best_floats >= 1 are required");
    KeepTable T{};
    int64_t longest = 0;
    for (int i = 0; i < n_entries; i++) {
        const MeshKeepEntry &e = entries_host[i];
        if (!e.src_dev || ((uintptr_t)e.src_dev & 3)) return fail(c, MESHENV_E_ARG, fn + ": entry " + std::to_string(i) + " has a NULL or misaligned source");
        if (e.numel < 1 || e.dst_offset < 0 || e.dst_offset > best_floats || e.numel > best_floats - e.dst_offset)
            return fail(c, MESHENV_E_ARG, fn + ": entry " + std::to_string(i) + " lies outside the " + std::to_string(best_floats) + " floats of best_dev");
        T.e[i].src = e.src_dev; T.e[i].dst_off = e.dst_offset; T.e[i].numel = e.numel;
        if (e.numel > longest) longest = e.numel;
    }
    const int64_t want = (longest / 4 + kKeepThreads - 1) / kKeepThreads + 1;   // one 16-byte copy per thread, the rest strides
    const int chunks = want < kKeepMaxChunks ? (int)want : kKeepMaxChunks;
    DeviceGuard guard(c->device);
    return launch(c, guard, "meshenv_keep_best", [&] {
        hipLaunchKernelGGL(k_keep_best, dim3(chunks, n_entries), dim3(kKeepThreads), 0, c->stream, best_dev, improved_dev, T);
    });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ the FNN mesher (include/meshenv_fnn.h)
struct MeshFnn : HandleBase {
    float *buf = nullptr;        // the packed weights, MESHENV_FNN_PACKED_FLOATS
    bool loaded = false;
    // meshenv_move_fnn_multi without histories: the points / types / code / done / complete of the step in flight
    char *scratch = nullptr;
    int scratch_envs = 0;
    PackTable table{};           // meshenv_fnn_bind: the live tensors and where meshenv_fnn_refresh packs them
    int n_copies = 0;
    bool live = false;
};

namespace {

static_assert(kFnnPackedFloats == MESHENV_FNN_PACKED_FLOATS, "csrc/meshenv_fnn.h and include/meshenv_fnn.h disagree");
static_assert(kMoveSkipped == MESHENV_MOVE_SKIPPED, "csrc/meshenv_kernels.h and include/meshenv_fnn.h disagree");

// rows of the seven layers, in MESHENV_FNN_TENSORS' order; the two heads are layer 5's rows 0-1 and 2-4
const int kFnnRows[7] = {64, 128, 64, 32, 16, kFnnAction, kFnnTypes};

// The FNN's buffer (MESHENV_FNN_PACKED_FLOATS), in MESHENV_FNN_TENSORS' order: layer l's weight tiles at fnn_w_offset(l), its bias
// behind them; the type_head sits behind the action_head in layer 5's tile.
PackLayout fnn_layout()
{
    PackLayout L;
    for (int i = 0; i < 7; i++) {
        const int l = i < 5 ? i : 5, row0 = i == 6 ? kFnnAction : 0;
        L.add(fnn_w_offset(l), kFnnRows[i], fnn_in(l), fnn_k(l) / 16, fnn_tiles(l), row0, kPackMatrix);
        L.add(fnn_b_offset(l), kFnnRows[i], 0, 0, 0, row0, kPackVector);
    }
    L.floats = kFnnPackedFloats;
    return L;
}

std::string fnn_pack(const float *const *tensors, const int32_t *shapes, float *out)
{
    if (!tensors || !shapes || !out) return "null pointer";
    for (int i = 0; i < 7; i++) {
        const int rows = kFnnRows[i], cols = fnn_in(i < 5 ? i : 5);
        if (!tensors[2 * i] || !tensors[2 * i + 1]) return "null tensor pointer";
        const int32_t *sw = shapes + 4 * i, *sb = sw + 2;
        if (sw[0] != rows || sw[1] != cols || sb[0] != rows || sb[1] != 1)
            return "tensor pair " + std::to_string(i) + " has shapes [" + std::to_string(sw[0]) + "][" + std::to_string(sw[1]) + "], [" +
                   std::to_string(sb[0]) + "]; " + kFnnShapes;
    }
    std::memset(out, 0, sizeof(float) * (size_t)kFnnPackedFloats);
    pack_host(fnn_layout(), tensors, out);
    return std::string();
}

int fnn_launch(MeshFnn *f, const char *fn, const FnnArgs &A)
{
    DeviceGuard guard(f->device);
    return launch(f, guard, fn, [&] {
        hipLaunchKernelGGL(k_fnn_forward, dim3((A.n + kFnnEnvs - 1) / kFnnEnvs), dim3(64 * kFnnWaves), 0, f->stream, A);
    });
}

}  // namespace

extern "C" {

int meshenv_fnn_create(int device, void *stream, MeshFnn **out) { return create_handle("meshenv_fnn_create", device, stream, out); }

void meshenv_fnn_destroy(MeshFnn *f)
{
    if (f && f->scratch) {
        DeviceGuard guard(f->device);
        (void)hipStreamSynchronize(f->stream);
        (void)hipFree(f->scratch);
    }
    destroy_handle(f, f ? f->buf : nullptr);
}

int meshenv_fnn_set_stream(MeshFnn *f, void *stream) { return set_stream(f, stream); }

const char *meshenv_fnn_last_error(const MeshFnn *f) { return last_error(f); }

int meshenv_fnn_pack(const float *const *tensors, const int32_t *shapes, float *out_host)
{
    const std::string refusal = fnn_pack(tensors, shapes, out_host);
    if (refusal.empty()) return MESHENV_OK;
    g_create_error = "meshenv_fnn_pack: " + refusal;
    return MESHENV_E_ARG;
}

int meshenv_fnn_load(MeshFnn *f, const float *const *tensors, const int32_t *shapes)
{
    if (!f) return MESHENV_E_ARG;
    std::vector<float> h((size_t)kFnnPackedFloats);
    const std::string refusal = fnn_pack(tensors, shapes, h.data());
    if (!refusal.empty()) return fail(f, MESHENV_E_ARG, "meshenv_fnn_load: " + refusal);
    DeviceGuard guard(f->device);
    if (guard.err != hipSuccess) return fail(f, MESHENV_E_HIP, "meshenv_fnn_load: hipSetDevice failed");
    (void)hipStreamSynchronize(f->stream);   // the previous weights may still be in use
    f->loaded = false;
    if ((!f->buf && hipMalloc((void **)&f->buf, h.size() * sizeof(float)) != hipSuccess) ||
        hipMemcpy(f->buf, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return fail(f, MESHENV_E_HIP, "meshenv_fnn_load: upload failed");
    f->loaded = true;
    return MESHENV_OK;
}

int meshenv_fnn_forward(MeshFnn *f, int n, const float *obs_dev, const uint8_t *finished_dev, double *points_dev,
                        double *types_dev, float *actions_dev, float *logits_dev)
{
    if (!f) return MESHENV_E_ARG;
    if (!f->loaded) return fail(f, MESHENV_E_STATE, "meshenv_fnn_forward: no weights loaded");
    if (n <= 0 || !obs_dev) return fail(f, MESHENV_E_ARG, "meshenv_fnn_forward: n > 0 and obs_dev are required");
    if (!points_dev && !types_dev && !actions_dev && !logits_dev) return fail(f, MESHENV_E_ARG, "meshenv_fnn_forward: no output requested");
    FnnArgs A{};
    A.packed = f->buf; A.n = n; A.obs = obs_dev; A.finished = finished_dev;
    A.points = points_dev; A.types = types_dev; A.actions = actions_dev; A.logits = logits_dev;
    return fnn_launch(f, "meshenv_fnn_forward", A);
}

int meshenv_move_fnn_multi(MeshEnv *h, MeshFnn *f, int T, float *obs_dev, uint8_t *finished_dev, int32_t *steps_dev,
                           uint8_t *done_dev, uint8_t *complete_dev, uint8_t *code_dev, int32_t *n_elements_dev,
                           double *hist_points_dev, double *hist_types_dev, float *hist_obs_dev, uint8_t *hist_code_dev,
                           uint8_t *hist_done_dev, uint8_t *hist_complete_dev)
{
    if (!h || !f) return MESHENV_E_ARG;
    if (T <= 0 || !obs_dev || !finished_dev || !steps_dev || !done_dev || !complete_dev || !code_dev)
        return fail_arg(h, "meshenv_move_fnn_multi: T > 0 and non-null obs, finished, steps, done, complete and code are required");
    if (!f->loaded) {
        h->err = "meshenv_move_fnn_multi: the network has no weights loaded";
        return MESHENV_E_STATE;
    }
    if (f->device != h->device || f->stream != h->stream) {   // the forward and move launches are ordered by the stream alone
        h->err = "meshenv_move_fnn_multi: env and network must be on the same device and stream (meshenv_set_stream / "
                 "meshenv_fnn_set_stream)";
        return MESHENV_E_STATE;
    }
    MESHENV_ON_DEVICE(h);
    const size_t n = (size_t)h->n_envs;
    if (f->scratch_envs < h->n_envs) {   // [n][2] + [n] doubles, 3 x [n] bytes
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (f->scratch) (void)hipFree(f->scratch);
        f->scratch = nullptr;
        f->scratch_envs = 0;
        HIP_TRY(h, hipMalloc((void **)&f->scratch, n * (3 * sizeof(double) + 3)));
        f->scratch_envs = h->n_envs;
    }
    double *s_points = (double *)f->scratch, *s_types = s_points + 2 * n;
    uint8_t *s_code = (uint8_t *)(s_types + n), *s_done = s_code + n, *s_complete = s_done + n;
    FnnArgs A{};
    A.packed = f->buf; A.n = (int)n; A.obs = obs_dev; A.finished = finished_dev;
    const int nb = (h->n_envs + 255) / 256;
    for (int t = 0; t < T; t++) {
        const size_t row = (size_t)t * n;
        A.points = hist_points_dev ? hist_points_dev + 2 * row : s_points;
        A.types = hist_types_dev ? hist_types_dev + row : s_types;
        A.obs_copy = hist_obs_dev ? hist_obs_dev + row * kObsDim : nullptr;
        uint8_t *code_t = hist_code_dev ? hist_code_dev + row : s_code;
        uint8_t *done_t = hist_done_dev ? hist_done_dev + row : s_done;
        uint8_t *complete_t = hist_complete_dev ? hist_complete_dev + row : s_complete;
        const bool timed = h->timing == 1 && !h->ev.empty();
        const size_t slot = (size_t)(h->ev_count % MESHENV_TIMING_POOL);
        if (timed) HIP_TRY(h, hipEventRecord(h->ev[2 * slot], h->stream));
        const int rf = fnn_launch(f, "meshenv_move_fnn_multi", A);
        if (rf != MESHENV_OK) {
            h->err = f->err;
            return rf;
        }
        if (timed) {
            HIP_TRY(h, hipEventRecord(h->ev[2 * slot + 1], h->stream));
            h->ev_count += 1;
        }
        const int rm = move_impl(h, A.points, A.types, obs_dev, done_t, complete_t, code_t, finished_dev);
        if (rm != MESHENV_OK) return rm;
        hipLaunchKernelGGL(k_fnn_advance, dim3(nb), dim3(256), 0, h->stream, h->S, finished_dev, steps_dev, (const uint8_t *)done_t,
                           (const uint8_t *)complete_t, (const uint8_t *)code_t, done_dev, complete_dev, code_dev, n_elements_dev);
        HIP_TRY(h, hipGetLastError());
    }
    return MESHENV_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ training the FNN mesher (include/meshenv_fnn_train.h)
static_assert(MESHENV_FNN_GRAD_FLOATS == FgLayout::stride && MESHENV_FNN_GRAD_OUTPUTS == kFgOut && MESHENV_FNN_GRAD_MAX_GROUPS == kCgMaxGroups,
              "include/meshenv_fnn_train.h and csrc/meshenv_fnn_grad.h disagree");
static_assert(2 * kFgLayers == MESHENV_FNN_TENSORS && MESHENV_FNN_TENSORS <= kTgtMaxCopies, "the copy table holds the 14 sources");

struct MeshFnnGrad : GradHandle {
    const float *w[kFgLayers]{}, *b[kFgLayers]{};
};

extern "C" {

int meshenv_fnn_grad_create(int device, void *stream, MeshFnnGrad **out)
{
    return create_handle("meshenv_fnn_grad_create", device, stream, out);
}

void meshenv_fnn_grad_destroy(MeshFnnGrad *g) { destroy_handle(g, g ? g->partial : nullptr); }

const char *meshenv_fnn_grad_last_error(const MeshFnnGrad *g) { return last_error(g); }

int meshenv_fnn_grad_set_stream(MeshFnnGrad *g, void *stream) { return set_stream(g, stream); }

int meshenv_fnn_grad_bind(MeshFnnGrad *g, const float *const *tensors_dev, float *grad_dev, int64_t n_grad)
{
    if (!g) return MESHENV_E_ARG;
    const int count = MESHENV_FNN_TENSORS;   // (the entry point takes no count)
    const int rc = grad_bind(g, kFnnGradBind, &tensors_dev, &count, grad_dev, n_grad, FgLayout::stride, (size_t)kCgMaxGroups * FgLayout::set);
    if (rc != MESHENV_OK) return rc;
    grad_bind_pairs(tensors_dev, kFgLayers, g->w, g->b);
    return MESHENV_OK;
}

int meshenv_fnn_grad_backward(MeshFnnGrad *g, int n, int N, const float *x_dev, const float *y_dev, const int32_t *rows_dev,
                              float *out_dev, float *accum_dev)
{
    static const char *fn = "meshenv_fnn_grad_backward";
    if (!g) return MESHENV_E_ARG;
    if (!g->bound) return fail(g, MESHENV_E_STATE, std::string(fn) + ": no tensors bound (meshenv_fnn_grad_bind)");
    if (n <= 0 || N <= 0 || N > (1 << 24) || n > (1 << 24) || !x_dev || !y_dev || !out_dev || (!rows_dev && n > N))
        return fail(g, MESHENV_E_ARG, std::string(fn) + ": 0 < n, N <= 2^24, n <= N without rows_dev, and x, y and out are required");
    FgArgs A{};
    A.n = n; A.N = N;
    A.nwg = fnn_grad_groups(n);
    A.x = x_dev; A.y = y_dev; A.rows = rows_dev;
    for (int l = 0; l < kFgLayers; l++) {
        A.w[l] = g->w[l];
        A.b[l] = g->b[l];
    }
    A.partial = g->partial;
    DeviceGuard guard(g->device);
    return launch_reduced(g, guard, fn, [&] { hipLaunchKernelGGL(k_fnn_grad, dim3(A.nwg), dim3(kFgThreads), 0, g->stream, A); }, [&] {
        hipLaunchKernelGGL(k_fnn_grad_reduce, dim3((FgLayout::params + 255) / 256), dim3(256), 0, g->stream, (const float *)g->partial,
                           A.nwg, g->grad, out_dev, accum_dev);
    });
}

// ---- live weights into a loaded FusedFNN (the twin of meshenv_policy_bind / meshenv_policy_refresh)
int meshenv_fnn_bind(MeshFnn *f, const float *const *tensors_dev)
{
    if (!f) return MESHENV_E_ARG;
    if (!f->loaded) return fail(f, MESHENV_E_STATE, "meshenv_fnn_bind: no weights loaded (meshenv_fnn_load lays the buffer out)");
    if (!tensors_dev) return fail(f, MESHENV_E_ARG, std::string("meshenv_fnn_bind: takes 14 tensors; ") + kFnnShapes);
    for (int i = 0; i < MESHENV_FNN_TENSORS; i++)
        if (!tensors_dev[i]) return fail(f, MESHENV_E_ARG, "meshenv_fnn_bind: null tensor");
    f->n_copies = pack_table(fnn_layout(), tensors_dev, MESHENV_FNN_TENSORS, f->buf, f->table);
    f->live = true;
    return MESHENV_OK;
}

int meshenv_fnn_refresh(MeshFnn *f)
{
    if (!f) return MESHENV_E_ARG;
    if (!f->loaded || !f->live) return fail(f, MESHENV_E_STATE, "meshenv_fnn_refresh: no tensors bound (meshenv_fnn_bind)");
    return pack_refresh(f, "meshenv_fnn_refresh");
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ synthetic training samples
static_assert(MESHENV_AUGMENT_PHILOX_TAG == kAugPhiloxTag && MESHENV_AUGMENT_BINS == kAugBins && MESHENV_AUGMENT_TYPES == kAugTypes &&
                  MESHENV_AUGMENT_MAX_ACTIONS == kAugMaxActions && MESHENV_AUGMENT_UNIFORMS == kAugMaxUniforms &&
                  (uint64_t)MESHENV_AUGMENT_MAX_ROUNDS * MESHENV_AUGMENT_MAX_ROUND < ((uint64_t)1 << 32),
              "include/meshenv_augment.h and csrc/meshenv_augment.h disagree");

struct MeshAugment : HandleBase {
    char *buf = nullptr;   // the per-bin tables, then flag / surv / acc of one round
    size_t cap = 0;
};

namespace {

size_t aug_align(size_t v) { return (v + 255) & ~(size_t)255; }

// rows a bin of type t owes: Q - 1 with Q = ceil(frac_t * (n / pool) / 11), data_augmentation.py:116, :137-139, :276-278, :963
int64_t aug_rows_per_bin(int64_t n, int pool, int t)
{
    const double per_worker = (double)n / (double)pool;
    const double q = std::ceil((t == 0 ? 0.5 : 0.25) * per_worker / 11);
    return q >= 1.0 ? (int64_t)q - 1 : 0;
}

}  // namespace

extern "C" {

int meshenv_augment_create(int device, void *stream, MeshAugment **out)
{
    const int rc = create_handle("meshenv_augment_create", device, stream, out);
    if (rc != MESHENV_OK) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess || upload_atan_state() != hipSuccess) {  // the tie-breaker of every quantised angle (atan2_x_nc)
        delete *out;
        *out = nullptr;
        g_create_error = "meshenv_augment_create: the atan2 state could not be uploaded";
        return MESHENV_E_HIP;
    }
    return MESHENV_OK;
}

void meshenv_augment_destroy(MeshAugment *a) { destroy_handle(a, a ? a->buf : nullptr); }

const char *meshenv_augment_last_error(const MeshAugment *a) { return last_error(a); }

int meshenv_augment_set_stream(MeshAugment *a, void *stream) { return set_stream(a, stream); }

int meshenv_augment_score(MeshAugment *a, int n, const double *obs_dev, const double *act_dev, double threshold,
                          uint8_t *rejected_dev, uint8_t *valid_dev, double *q_dev, uint8_t *accept_dev)
{
    if (!a) return MESHENV_E_ARG;
    const char *fn = "meshenv_augment_score";
    if (n < 0 || n > (1 << 24) || !obs_dev || !act_dev || !rejected_dev || !valid_dev || !q_dev)
        return fail(a, MESHENV_E_ARG, std::string(fn) + ": 0 <= n <= 2^24, and obs, act, rejected, valid and q are required");
    if (accept_dev && !(threshold > 0.0 && threshold <= 1.0))
        return fail(a, MESHENV_E_ARG, std::string(fn) + ": threshold outside (0, 1]");
    if (n == 0) return MESHENV_OK;
    DeviceGuard guard(a->device);
    return launch(a, guard, fn, [&] {
        hipLaunchKernelGGL(k_aug_score_rows, dim3((n + kAugThreads - 1) / kAugThreads), dim3(kAugThreads), 0, a->stream, n, obs_dev,
                           act_dev, threshold, rejected_dev, valid_dev, q_dev, accept_dev);
    });
}

int meshenv_augment_propose(MeshAugment *a, int n, const double *uniforms_dev, const int32_t *t_dev, const int32_t *b_dev,
                            const int32_t *t_host, const int32_t *b_host, double *angle_dev, double *obs_dev, double *act_dev,
                            uint8_t *rejected_dev)
{
    if (!a) return MESHENV_E_ARG;
    const char *fn = "meshenv_augment_propose";
    if (n < 0 || n > (1 << 24) || !uniforms_dev || !t_dev || !b_dev || !t_host || !b_host || !angle_dev || !obs_dev || !act_dev ||
        !rejected_dev)
        return fail(a, MESHENV_E_ARG, std::string(fn) + ": 0 <= n <= 2^24 and every pointer is required");
    for (int i = 0; i < n; i++)
        if (t_host[i] < 0 || t_host[i] >= kAugTypes || b_host[i] < 0 || b_host[i] >= kAugBins)
            return fail(a, MESHENV_E_ARG, std::string(fn) + ": row " + std::to_string(i) + ": type index outside 0..2 or bin outside 0..10");
    if (n == 0) return MESHENV_OK;
    DeviceGuard guard(a->device);
    return launch(a, guard, fn, [&] {
        hipLaunchKernelGGL(k_aug_propose_recorded, dim3((n + kAugThreads - 1) / kAugThreads), dim3(kAugThreads), 0, a->stream, n,
                           uniforms_dev, t_dev, b_dev, angle_dev, obs_dev, act_dev, rejected_dev);
    });
}

int meshenv_augment_sample(MeshAugment *a, int64_t n, double threshold, uint64_t seed, int pool, int round_size, int max_rounds,
                           int64_t rows, double *x64_dev, double *y64_dev, float *x32_dev, float *y32_dev, int32_t *counts_host,
                           uint64_t *stats_host)
{
    if (!a) return MESHENV_E_ARG;
    const std::string fn = "meshenv_augment_sample";
    if (n < 0 || n > ((int64_t)1 << 40) || pool < 1 || pool > MESHENV_AUGMENT_MAX_POOL)
        return fail(a, MESHENV_E_ARG, fn + ": 0 <= n <= 2^40 and 1 <= pool <= 1024");
    if (!(threshold > 0.0 && threshold <= 1.0)) return fail(a, MESHENV_E_ARG, fn + ": threshold outside (0, 1]");
    if (round_size < 64 || round_size > MESHENV_AUGMENT_MAX_ROUND || round_size % 64 || max_rounds < 1 || max_rounds > MESHENV_AUGMENT_MAX_ROUNDS)
        return fail(a, MESHENV_E_ARG, fn + ": 64 <= round_size <= 2^20 in multiples of 64, 1 <= max_rounds <= 4095");
    if ((!x64_dev) != (!y64_dev) || (!x32_dev) != (!y32_dev) || (!x64_dev && !x32_dev))
        return fail(a, MESHENV_E_ARG, fn + ": x and y come in pairs, and the float64 or the float32 pair is required");
    const int G = pool * kAugTypes * kAugBins;
    std::vector<int32_t> owed(G);
    std::vector<int64_t> row0(G);
    int64_t total = 0, acc_cap = 0;
    for (int g = 0; g < G; g++) {
        const int t = (g / kAugBins) % kAugTypes;
        const int64_t r = aug_rows_per_bin(n, pool, t);
        if (r > INT32_MAX || total + r > ((int64_t)1 << 40)) return fail(a, MESHENV_E_ARG, fn + ": too many rows");
        owed[g] = (int32_t)r;
        row0[g] = total;
        total += r;
        acc_cap += (int64_t)round_size * (t == 0 ? kAugMaxActions : 1);
    }
    if (rows != total)
        return fail(a, MESHENV_E_ARG, fn + ": these arguments give " + std::to_string((long long)total) + " rows, the buffers have " +
                       std::to_string((long long)rows));
    if (stats_host) std::memset(stats_host, 0, sizeof(uint64_t) * MESHENV_AUGMENT_STATS);
    if (counts_host) std::memset(counts_host, 0, sizeof(int32_t) * (size_t)G);
    if (total == 0) return MESHENV_OK;

    // one allocation: rows, row0 | count, next_p, n_surv, tally | active, acc_at of the round | flag, surv, acc of the round.
    // A round has lanes = G * round_size proposals and acc_cap candidates, however many bins share them.
    const int64_t lanes = (int64_t)G * round_size;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = aug_align(at + bytes); return o; };
    const size_t o_rows = take(sizeof(int32_t) * G), o_row0 = take(sizeof(int64_t) * G);
    const size_t tables_end = at;
    const size_t o_count = take(sizeof(int32_t) * G), o_next = take(sizeof(uint32_t) * G), o_nsurv = take(sizeof(int32_t) * G);
    const size_t o_tally = take(sizeof(unsigned long long) * 2 * G);
    const size_t zero_end = at;
    const size_t o_active = take(sizeof(int32_t) * G), o_acc_at = take(sizeof(int64_t) * ((size_t)G + 1));
    const size_t o_flag = take((size_t)lanes), o_surv = take(sizeof(int32_t) * (size_t)lanes);
    const size_t o_acc = take((size_t)acc_cap);
    if (at > ((size_t)8 << 30)) return fail(a, MESHENV_E_ARG, fn + ": pool * round_size needs more than 8 GiB of scratch");
    DeviceGuard guard(a->device);
    if (guard.err != hipSuccess) return fail(a, MESHENV_E_HIP, fn + ": hipSetDevice failed");
    if (at > a->cap) {
        if (hipStreamSynchronize(a->stream) != hipSuccess) return fail(a, MESHENV_E_HIP, fn + ": hipStreamSynchronize failed");
        if (a->buf) (void)hipFree(a->buf);
        a->buf = nullptr;
        a->cap = 0;
        if (hipMalloc((void **)&a->buf, at) != hipSuccess) return fail(a, MESHENV_E_HIP, fn + ": allocation failed");
        a->cap = at;
    }
    std::vector<char> tables(tables_end);
    std::memcpy(tables.data() + o_rows, owed.data(), sizeof(int32_t) * G);
    std::memcpy(tables.data() + o_row0, row0.data(), sizeof(int64_t) * G);
    if (hipMemcpyAsync(a->buf, tables.data(), tables_end, hipMemcpyHostToDevice, a->stream) != hipSuccess ||
        hipMemsetAsync(a->buf + tables_end, 0, zero_end - tables_end, a->stream) != hipSuccess ||
        hipStreamSynchronize(a->stream) != hipSuccess)
        return fail(a, MESHENV_E_HIP, fn + ": upload failed");

    AugRound A{};
    A.seed = seed;
    A.threshold = threshold;
    A.rows = (const int32_t *)(a->buf + o_rows);
    A.row0 = (const int64_t *)(a->buf + o_row0);
    A.count = (int32_t *)(a->buf + o_count);
    A.next_p = (uint32_t *)(a->buf + o_next);
    A.n_surv = (int32_t *)(a->buf + o_nsurv);
    A.tally = (unsigned long long *)(a->buf + o_tally);
    A.active = (const int32_t *)(a->buf + o_active);
    A.acc_at = (const int64_t *)(a->buf + o_acc_at);
    A.flag = (uint8_t *)(a->buf + o_flag);
    A.surv = (int32_t *)(a->buf + o_surv);
    A.acc = (uint8_t *)(a->buf + o_acc);
    A.x64 = x64_dev; A.y64 = y64_dev; A.x32 = x32_dev; A.y32 = y32_dev;

    std::vector<int32_t> count(G, 0), active(G);
    std::vector<int64_t> acc_at((size_t)G + 1);
    int rounds = 0;
    bool done = false;
    while (!done && rounds < max_rounds) {
        // the unfinished bins share the round's lanes and candidates: P = what fits, a multiple of 64, at most 2^20
        int n_active = 0;
        int64_t actions = 0;
        for (int g = 0; g < G; g++)
            if (count[g] < owed[g]) {
                active[n_active++] = g;
                actions += (g / kAugBins) % kAugTypes == 0 ? kAugMaxActions : 1;
            }
        int64_t P = std::min<int64_t>(lanes / n_active, acc_cap / actions);
        P = std::min<int64_t>(P / kAugThreads * kAugThreads, MESHENV_AUGMENT_MAX_ROUND);   // >= round_size: every subset fits
        int64_t acc_total = 0;
        for (int i = 0; i < n_active; i++) {
            acc_at[i] = acc_total;
            acc_total += P * ((active[i] / kAugBins) % kAugTypes == 0 ? kAugMaxActions : 1);
        }
        acc_at[n_active] = acc_total;
        A.n_active = n_active;
        A.P = (int)P;
        // (pageable memory: the two vectors are not written again before the synchronise that ends the round)
        if (hipMemcpyAsync(a->buf + o_active, active.data(), sizeof(int32_t) * n_active, hipMemcpyHostToDevice, a->stream) != hipSuccess ||
            hipMemcpyAsync(a->buf + o_acc_at, acc_at.data(), sizeof(int64_t) * ((size_t)n_active + 1), hipMemcpyHostToDevice, a->stream) != hipSuccess)
            return fail(a, MESHENV_E_HIP, fn + ": uploading the round's slots failed");
        const dim3 grid_p((unsigned)(P / kAugThreads), n_active);
        const dim3 grid_s((unsigned)(acc_total / kAugThreads));
        int rc = launch(a, guard, fn.c_str(), [&] { hipLaunchKernelGGL(k_aug_propose, grid_p, dim3(kAugThreads), 0, a->stream, A); }, "proposal launch");
        if (rc == MESHENV_OK)
            rc = launch(a, guard, fn.c_str(), [&] { hipLaunchKernelGGL(k_aug_compact, dim3(n_active), dim3(kAugScanThreads), 0, a->stream, A); }, "compaction launch");
        if (rc == MESHENV_OK)
            rc = launch(a, guard, fn.c_str(), [&] { hipLaunchKernelGGL(k_aug_score, grid_s, dim3(kAugThreads), 0, a->stream, A); }, "scoring launch");
        if (rc == MESHENV_OK)
            rc = launch(a, guard, fn.c_str(), [&] { hipLaunchKernelGGL(k_aug_select, dim3(n_active), dim3(kAugScanThreads), 0, a->stream, A); }, "selection launch");
        if (rc != MESHENV_OK) return rc;
        rounds++;
        if (hipMemcpyAsync(count.data(), A.count, sizeof(int32_t) * G, hipMemcpyDeviceToHost, a->stream) != hipSuccess ||
            hipStreamSynchronize(a->stream) != hipSuccess)
            return fail(a, MESHENV_E_HIP, fn + ": reading the counts failed");
        done = true;
        for (int g = 0; g < G; g++) done = done && count[g] >= owed[g];
    }
    if (counts_host) std::memcpy(counts_host, count.data(), sizeof(int32_t) * (size_t)G);
    if (stats_host) {
        std::vector<unsigned long long> tally(2 * (size_t)G);
        if (hipMemcpy(tally.data(), A.tally, sizeof(unsigned long long) * tally.size(), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(a, MESHENV_E_HIP, fn + ": reading the tallies failed");
        for (int g = 0; g < G; g++) {
            stats_host[0] += tally[2 * (size_t)g];
            stats_host[1] += tally[2 * (size_t)g + 1];
            stats_host[2] += (uint64_t)count[g];
        }
        stats_host[3] = (uint64_t)rounds;
    }
    if (!done) {
        int shortfall = 0;
        for (int g = 0; g < G; g++) shortfall += count[g] < owed[g];
        return fail(a, MESHENV_E_RANGE, fn + ": " + std::to_string(shortfall) + " of " + std::to_string(G) + " bins are short after " +
                       std::to_string(rounds) + " rounds of " + std::to_string((long long)lanes) + " proposals");
    }
    return MESHENV_OK;
}

}  // extern "C"
