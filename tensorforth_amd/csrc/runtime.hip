// runtime.hip - device selection, HBM allocation, copies, streams, events, hipGraph capture.
// Replaces the reference's cudaSetDevice / cudaMallocManaged arena / cudaMemcpy /
// cudaDeviceSynchronize plumbing (src/ten4.cu:125-152, src/mu/mmu.cu:44-46,
// src/ten4_types.h:186-201).
#include "t4k_common.h"
#include <stdarg.h>
#include <string.h>
#include <algorithm>

namespace t4k {

State &st() { static State s; return s; }

int fail(int code, const char *fmt, ...) {
    va_list ap; va_start(ap, fmt);
    vsnprintf(st().err, sizeof(st().err), fmt, ap);
    va_end(ap);
    return code;
}
void conv_plan_note(const char *fmt, ...) {
    State &g = st();
    if (g.conv_plan_depth <= 0 || g.conv_plan_len >= (int)sizeof(g.conv_plan) - 1) return;
    if (g.conv_plan_len) g.conv_plan[g.conv_plan_len++] = ' ';
    va_list ap; va_start(ap, fmt);
    const int n = vsnprintf(g.conv_plan + g.conv_plan_len, sizeof(g.conv_plan) - g.conv_plan_len, fmt, ap);
    va_end(ap);
    if (n > 0) g.conv_plan_len = std::min(g.conv_plan_len + n, (int)sizeof(g.conv_plan) - 1);
}
int hip_fail(hipError_t e, const char *what) {
    snprintf(st().err, sizeof(st().err), "HIP error %d (%s) at %s", (int)e, hipGetErrorString(e), what);
    return T4K_ERR_HIP;
}

} // namespace t4k

using namespace t4k;

namespace t4k { void rng_sync_device(hipStream_t hs); }   // optim.hip
namespace t4k {
int spin_check() {
    State &g = st();
    if (!g.spin_err) return T4K_OK;
    const int code = *(volatile int *)g.spin_err;
    if (!code) return T4K_OK;
    *(volatile int *)g.spin_err = 0;
    // what waited, and the switch that takes that path out (t4k.h / DESIGN.md section 9)
    static const char *what[] = { "unknown wait", "dual GEMM writer gate", "dual-GEMM epoch slots", "pair-mode GEMM flag", "head backward dW gate",
                                  "head backward staging gate", "column-sliced head backward target store", "conv-stack head band exchange", "fused head backward target store",
                                  "one-shot gradient exchange: a peer's element never arrived" };
    static const char *off[]  = { "T4K_GEMM_DUAL=0 T4K_GEMM_DUAL32=0 T4K_LINSMALL_GATE=0 T4_STACK_HEAD=0 T4_HEAD_BWD=0", "T4K_GEMM_DUAL=0", "T4K_GEMM_DUAL32=0", "T4K_GEMM_PLAIN_PAIR=0",
                                  "T4K_LINSMALL_GATE=0", "T4K_LINSMALL_GATE=0", "T4K_LINSMALL_COLS=0", "T4_STACK_HEAD=0 (or T4K_STACK_HEAD=0)", "T4_HEAD_BWD=0 (or T4K_HEAD_BWD=0)",
                                  "T4_DP_XCHG=0 (the slab then goes through RCCL); check that every rank reached the optimizer" };
    const int k = (code > 0 && code < 10) ? code : 0;
    // Degrade, do not keep failing: from here on the launchers pick only kernels whose workgroups never wait for each other
    // (the per-layer / split paths: more launches, same results) - a partitioned or shared device then costs speed, not correctness.  The exchange of a
    // data-parallel job (code 9) is another matter: a peer is missing, nothing local can replace it.
    if (k != 9) g.gates_off = true;
    return fail(T4K_ERR_HIP, "an inter-workgroup wait timed out (code %d: %s): the launch's workgroups were not co-resident - results of that launch are invalid%s; "
                             "on a shared or partitioned device set %s (or call t4k_gates_enable(0) up front)", code, what[k],
                             k != 9 ? "; the library now uses its ungated kernels (slower, correct) until t4k_gates_enable(1)" : "", off[k]);
}
}
namespace { struct GraphRec { hipGraphExec_t exec; uint64_t rng_adv; }; }

extern "C" {

int t4k_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int t4k_init(int device) {
    State &g = st();
    if (g.ready && g.device == device) return T4K_OK;
    int n = t4k_device_count();
    if (n <= 0) return fail(T4K_ERR_NODEVICE, "no HIP device visible: libt4hip has no CPU fallback");
    if (device < 0 || device >= n) return fail(T4K_ERR_ARG, "device %d out of range [0,%d)", device, n);
    T4K_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    T4K_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(T4K_ERR_NODEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    g.cu_count = prop.multiProcessorCount;
    if (!g.stream) { T4K_HIP(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking)); g.own_stream = true; }
    if (!g.ws) {
        g.ws_bytes = WS_BYTES;                         // 64 MiB: reductions, split-K slabs, linalg
        T4K_HIP(hipMalloc(&g.ws, g.ws_bytes));
        T4K_HIP(hipMemsetAsync(g.ws, 0, g.ws_bytes, g.stream));
    }
    // (zeroed on the library stream: a null-stream hipMemset is not ordered with a non-blocking stream's kernels)
    if (!g.d_zero) { T4K_HIP(hipMalloc((void **)&g.d_zero, 4096)); T4K_HIP(hipMemsetAsync(g.d_zero, 0, 4096, g.stream)); }
    if (!g.d_sync) { T4K_HIP(hipMalloc((void **)&g.d_sync, 32768 * sizeof(int))); T4K_HIP(hipMemsetAsync(g.d_sync, 0, 32768 * sizeof(int), g.stream)); }
    T4K_HIP(hipStreamSynchronize(g.stream));            // ... and complete before any stream (a caller's own, t4k_set_default_stream) can launch
    if (!g.spin_err) {                                  // error word of the bounded inter-workgroup waits: pinned host memory the kernels can write
        T4K_HIP(hipHostMalloc((void **)&g.spin_err, 64, hipHostMallocMapped)); *g.spin_err = 0;
        gemm_set_spin_err(g.spin_err); linear_set_spin_err(g.spin_err); linsmall_set_spin_err(g.spin_err);
    }
    g.device = device;
    g.ready  = true;
    return T4K_OK;
}

void t4k_shutdown(void) {
    State &g = st();
    if (!g.ready) return;
    (void)hipDeviceSynchronize();
    if (g.ws) { (void)hipFree(g.ws); g.ws = nullptr; }
    if (g.own_stream && g.stream) { (void)hipStreamDestroy(g.stream); }
    g.stream = nullptr; g.own_stream = false;
    g.pending = 0;                 // deferred work dies with its workspace and stream (a later t4k_init must not flush into freed memory)
    (void)t4k_xchg_destroy();
    g.ready = false;
}

int t4k_gates_enable(int on) { st().gates_off = !on; return T4K_OK; }
int t4k_gates_enabled(void) { return st().gates_off ? 0 : 1; }
const char *t4k_last_error(void)  { return st().err; }
unsigned long long t4k_launch_count(void) { return st().launches; }
const char *t4k_backend_name(void) { return "hip-gfx950"; }
const char *t4k_conv_last_plan(void) {
    static char text[sizeof(State::conv_plan)];
    memcpy(text, st().conv_plan, sizeof(text));
    return text;
}

int t4k_device_info(int *cu_count, int *clock_khz, size_t *hbm_bytes) {
    T4K_REQUIRE_INIT();
    hipDeviceProp_t prop;
    T4K_HIP(hipGetDeviceProperties(&prop, st().device));
    if (cu_count)  *cu_count  = prop.multiProcessorCount;
    if (clock_khz) *clock_khz = prop.clockRate;
    if (hbm_bytes) *hbm_bytes = prop.totalGlobalMem;
    return T4K_OK;
}

int t4k_malloc(void **p, size_t bytes) {
    T4K_REQUIRE_INIT();
    if (!p) return fail(T4K_ERR_ARG, "t4k_malloc: null");
    hipError_t e = hipMalloc(p, bytes ? bytes : 4);
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(T4K_ERR_NOMEM, "out of HBM (%zu bytes)", bytes); }
    T4K_HIP(e);
    return T4K_OK;
}
int t4k_free(void *p) { T4K_REQUIRE_INIT(); if (p) T4K_HIP(hipFree(p)); return T4K_OK; }
int t4k_host_alloc(void **p, size_t bytes) { T4K_REQUIRE_INIT(); T4K_HIP(hipHostMalloc(p, bytes ? bytes : 4, hipHostMallocDefault)); return T4K_OK; }
int t4k_host_free(void *p) { T4K_REQUIRE_INIT(); if (p) T4K_HIP(hipHostFree(p)); return T4K_OK; }

int t4k_memcpy_h2d(void *dst, const void *src, size_t bytes, t4k_stream_t s) {
    T4K_REQUIRE_INIT(); if (!bytes) return T4K_OK;
    T4K_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, S(s)));
    return T4K_OK;
}
int t4k_memcpy_d2h(void *dst, const void *src, size_t bytes, t4k_stream_t s) {
    T4K_REQUIRE_INIT(); if (!bytes) return T4K_OK;
    T4K_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, S(s)));
    return T4K_OK;
}
int t4k_memcpy_d2d(void *dst, const void *src, size_t bytes, t4k_stream_t s) {
    T4K_REQUIRE_INIT(); if (!bytes) return T4K_OK;
    T4K_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, S(s)));
    return T4K_OK;
}
int t4k_memset(void *dst, int byte, size_t bytes, t4k_stream_t s) {
    T4K_REQUIRE_INIT(); if (!bytes) return T4K_OK;
    T4K_HIP(hipMemsetAsync(dst, byte, bytes, S(s)));
    return T4K_OK;
}
int t4k_sync(t4k_stream_t s) { T4K_REQUIRE_INIT(); T4K_HIP(hipStreamSynchronize(S(s))); return spin_check(); }

int t4k_stream_create(t4k_stream_t *s) {
    T4K_REQUIRE_INIT();
    State &g = st();
    if (g.n_lane >= 8) return fail(T4K_ERR_NOMEM, "t4k_stream_create: at most 8 library streams");
    hipStream_t h; T4K_HIP(hipStreamCreateWithFlags(&h, hipStreamNonBlocking)); *s = (t4k_stream_t)h;
    void *ws = nullptr;                                 // every library stream owns a workspace (concurrent split-K / partial slabs)
    T4K_HIP(hipMalloc(&ws, g.ws_bytes)); T4K_HIP(hipMemsetAsync(ws, 0, g.ws_bytes, h));
    g.lane[g.n_lane].s = h; g.lane[g.n_lane].ws = ws; g.n_lane++;
    return T4K_OK;
}
int t4k_stream_create_plain(t4k_stream_t *s) {
    T4K_REQUIRE_INIT();
    hipStream_t h; T4K_HIP(hipStreamCreateWithFlags(&h, hipStreamNonBlocking)); *s = (t4k_stream_t)h;
    return T4K_OK;
}
int t4k_stream_destroy(t4k_stream_t s) {
    T4K_REQUIRE_INIT(); if (!s) return T4K_OK;
    State &g = st();
    T4K_HIP(hipStreamSynchronize((hipStream_t)s));
    for (int i = 0; i < g.n_lane; i++) if (g.lane[i].s == (hipStream_t)s) { (void)hipFree(g.lane[i].ws); g.lane[i] = g.lane[--g.n_lane]; break; }
    T4K_HIP(hipStreamDestroy((hipStream_t)s));
    return T4K_OK;
}
int t4k_stream_wait_event(t4k_stream_t s, t4k_event_t e) { T4K_REQUIRE_INIT(); T4K_HIP(hipStreamWaitEvent(S(s), (hipEvent_t)e, 0)); return T4K_OK; }
int t4k_set_default_stream(t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    State &g = st();
    if (g.own_stream && g.stream && g.stream != (hipStream_t)s) { (void)hipStreamSynchronize(g.stream); (void)hipStreamDestroy(g.stream); }
    g.stream = (hipStream_t)s; g.own_stream = false;
    return T4K_OK;
}
t4k_stream_t t4k_default_stream(void) { return (t4k_stream_t)st().stream; }

int t4k_event_create(t4k_event_t *e) { T4K_REQUIRE_INIT(); hipEvent_t h; T4K_HIP(hipEventCreate(&h)); *e = (t4k_event_t)h; return T4K_OK; }
int t4k_event_record(t4k_event_t e, t4k_stream_t s) { T4K_REQUIRE_INIT(); T4K_HIP(hipEventRecord((hipEvent_t)e, S(s))); return T4K_OK; }
int t4k_event_sync(t4k_event_t e) { T4K_REQUIRE_INIT(); T4K_HIP(hipEventSynchronize((hipEvent_t)e)); return spin_check(); }
// the wait of a HELPER thread (the dataset reader): nothing but the wait - it neither runs deferred work of the thread that drives the model nor
// reads / clears the wait-error word, which stays for that thread's next synchronising call
int t4k_event_wait(t4k_event_t e) { T4K_REQUIRE_INIT_NOFLUSH(); T4K_HIP(hipEventSynchronize((hipEvent_t)e)); return T4K_OK; }
int t4k_event_elapsed_ms(t4k_event_t a, t4k_event_t b, float *ms) { T4K_REQUIRE_INIT(); T4K_HIP(hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b)); return T4K_OK; }
int t4k_event_destroy(t4k_event_t e) { T4K_REQUIRE_INIT(); if (e) T4K_HIP(hipEventDestroy((hipEvent_t)e)); return T4K_OK; }

int t4k_graph_begin(t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    State &g = st();
    if (!g.d_rng) { T4K_HIP(hipMalloc((void **)&g.d_rng, 4 * sizeof(uint64_t))); T4K_HIP(hipMemsetAsync(g.d_rng, 0, 4 * sizeof(uint64_t), S(s))); g.d_rng_ctr = ~0ull; }
    T4K_HIP(hipStreamBeginCapture(S(s), hipStreamCaptureModeThreadLocal));
    g.capturing = true; g.cap_adv = 0;                  // draws recorded from here on read / advance the device copy of the stream
    return T4K_OK;
}
int t4k_graph_end(t4k_stream_t s, t4k_graph_t *out) {
    T4K_REQUIRE_INIT();
    State &g = st();
    g.capturing = false;
    hipGraph_t graph = nullptr;
    T4K_HIP(hipStreamEndCapture(S(s), &graph));
    hipGraphExec_t exec = nullptr;
    hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    T4K_HIP(e);
    *out = (t4k_graph_t) new GraphRec{ exec, g.cap_adv };   // remember how far one replay moves the Philox stream
    return T4K_OK;
}
int t4k_graph_launch(t4k_graph_t h, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!h) return fail(T4K_ERR_ARG, "t4k_graph_launch: null graph");
    GraphRec *r = (GraphRec *)h;
    State &g = st();
    if (r->rng_adv) rng_sync_device(S(s));               // the replay draws from the device copy: make it current first
    T4K_HIP(hipGraphLaunch(r->exec, S(s)));
    if (r->rng_adv) { g.rng_ctr += r->rng_adv; g.d_rng_ctr = g.rng_ctr; }   // the graph's kernels advance the device copy by the same amount
    return T4K_OK;
}
int t4k_graph_destroy(t4k_graph_t h) {
    T4K_REQUIRE_INIT();
    if (h) { GraphRec *r = (GraphRec *)h; T4K_HIP(hipGraphExecDestroy(r->exec)); delete r; }
    return T4K_OK;
}

} // extern "C"
