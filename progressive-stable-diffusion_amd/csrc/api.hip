// Library-level entry points: error text, device info, hipGraph capture, HIP-event profiling.
#include <stdarg.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dadd_common.h"

int dadd_init_igemm();
int dadd_init_attention();
int dadd_init_norm();
int dadd_init_attn2_fused();
int dadd_init_ffn_block();
int dadd_init_tf_head();
int dadd_init_attn_grad();        // training backward of attention (attn_grad.hip)
int dadd_init_igemm_bf16();      // the bf16 twins (*_bf16.hip)
int dadd_init_attention_bf16();
int dadd_init_norm_bf16();
int dadd_init_attn_grad_bf16();

namespace {
thread_local char g_err[512] = "";

struct ProfRec {
  const char* name;
  double flop, bytes;
};
struct ProfState {
  std::vector<hipEvent_t> ev;  // pairs (start, stop), reused across sessions
  std::vector<ProfRec> rec;
  std::vector<float> ms;       // filled by dadd_prof_end
} g_prof;
}  // namespace

int g_dadd_prof_on = 0;

void dadd_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

bool dadd_prof_slot(const DaddLaunchTag& tag, hipEvent_t* e0, hipEvent_t* e1) {
  const size_t i = g_prof.rec.size();
  while (g_prof.ev.size() < 2 * (i + 1)) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return false;
    g_prof.ev.push_back(e);
  }
  *e0 = g_prof.ev[2 * i];
  *e1 = g_prof.ev[2 * i + 1];
  g_prof.rec.push_back(ProfRec{tag.name, tag.flop, tag.bytes});
  return true;
}

extern "C" {

const char* dadd_last_error(void) { return g_err; }

int dadd_version(void) { return 100; }

int dadd_init(void) {
  int rc = dadd_init_igemm();
  if (rc == DADD_OK) rc = dadd_init_attention();
  if (rc == DADD_OK) rc = dadd_init_norm();
  if (rc == DADD_OK) rc = dadd_init_attn2_fused();
  if (rc == DADD_OK) rc = dadd_init_ffn_block();
  if (rc == DADD_OK) rc = dadd_init_igemm_bf16();
  if (rc == DADD_OK) rc = dadd_init_attention_bf16();
  if (rc == DADD_OK) rc = dadd_init_norm_bf16();
  if (rc == DADD_OK) rc = dadd_init_attn_grad();
  if (rc == DADD_OK) rc = dadd_init_attn_grad_bf16();
  return rc != DADD_OK ? rc : dadd_init_tf_head();
}

int dadd_device_info(int device, int64_t out[4]) {
  DADD_REQUIRE(out != nullptr, "device_info: null out");
  hipDeviceProp_t prop;
  DADD_HIP(hipGetDeviceProperties(&prop, device));
  out[0] = prop.multiProcessorCount;
  out[1] = (int64_t)prop.maxSharedMemoryPerMultiProcessor;
  out[2] = prop.clockRate;
  int arch = 0;
  const char* g = strstr(prop.gcnArchName, "gfx");
  if (g) arch = atoi(g + 3);
  out[3] = arch;
  return DADD_OK;
}

// ---- weight prefetch on a side branch ------------------------------------------------------------------------------------
// Every layer's weights are cold when its kernel starts (1.76 GB of UNet weights per step against 256 MB of Infinity
// Cache): 3-8 us of a GEMM launch are the first misses of its weight stream (profiles/r03_zg_cold_hot_weights.txt).
// dadd_prefetch() reads a weight tensor on a SIDE stream that forks from `stream` at the call (event) - inside a stream
// capture that is a parallel branch of the graph, running beside the kernels that precede the consumer - and
// dadd_prefetch_join() makes `stream` wait for the branch (before the capture ends / the results are used).  The reads
// leave the lines in the memory-side Infinity Cache, which every XCD hits.
namespace {
hipStream_t g_pf_stream = nullptr;
constexpr int PF_EVENTS = 64;
hipEvent_t g_pf_ev[PF_EVENTS];
int g_pf_next = 0;
bool g_pf_open = false;

__global__ __launch_bounds__(256) void prefetch_kernel(const uint4* __restrict__ p, size_t n16, unsigned* __restrict__ sink) {
  unsigned acc = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) {
    const uint4 v = p[i];
    acc ^= v.x ^ v.y ^ v.z ^ v.w;
  }
  if (acc == 0x9e3779b9u && sink != nullptr) *sink = acc;      // (never both: keeps the loads alive)
}

int pf_init() {
  if (g_pf_stream != nullptr) return DADD_OK;
  DADD_HIP(hipStreamCreateWithFlags(&g_pf_stream, hipStreamNonBlocking));
  for (int i = 0; i < PF_EVENTS; ++i) DADD_HIP(hipEventCreateWithFlags(&g_pf_ev[i], hipEventDisableTiming));
  return DADD_OK;
}
}  // namespace

int dadd_prefetch(const void* ptr, int64_t bytes, void* stream) {
  DADD_REQUIRE(ptr != nullptr && bytes >= 0 && dadd_aligned16(ptr), "prefetch: null / unaligned pointer");
  if (bytes < 16) return DADD_OK;
  int rc = pf_init();
  if (rc != DADD_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipEvent_t e = g_pf_ev[g_pf_next];
  g_pf_next = (g_pf_next + 1) % PF_EVENTS;
  DADD_HIP(hipEventRecord(e, s));                       // fork: the branch starts when `stream` reaches this point
  DADD_HIP(hipStreamWaitEvent(g_pf_stream, e, 0));
  const size_t n16 = (size_t)bytes / 16;
  int blocks = (int)((n16 + 256 * 16 - 1) / (256 * 16));    // >= 16 loads per thread, at most 48 workgroups
  if (blocks > 48) blocks = 48;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(prefetch_kernel, dim3(blocks), dim3(256), 0, g_pf_stream, static_cast<const uint4*>(ptr), n16,
                     static_cast<unsigned*>(nullptr));
  DADD_LAUNCH_CHECK();
  g_pf_open = true;
  return DADD_OK;
}

int dadd_prefetch_join(void* stream) {
  if (!g_pf_open) return DADD_OK;
  hipEvent_t e = g_pf_ev[g_pf_next];
  g_pf_next = (g_pf_next + 1) % PF_EVENTS;
  DADD_HIP(hipEventRecord(e, g_pf_stream));
  DADD_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(stream), e, 0));
  g_pf_open = false;
  return DADD_OK;
}

int dadd_graph_begin(void* stream) {
  DADD_REQUIRE(g_dadd_prof_on == 0, "graph_begin: profiling is active");
  DADD_HIP(hipStreamBeginCapture(static_cast<hipStream_t>(stream), hipStreamCaptureModeThreadLocal));
  return DADD_OK;
}

int dadd_graph_end(void* stream, void** graph_exec_out) {
  DADD_REQUIRE(graph_exec_out != nullptr, "graph_end: null out");
  hipGraph_t graph = nullptr;
  DADD_HIP(hipStreamEndCapture(static_cast<hipStream_t>(stream), &graph));
  hipGraphExec_t exec = nullptr;
  hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e != hipSuccess) {
    dadd_set_error("hipGraphInstantiate failed: %s", hipGetErrorString(e));
    return DADD_EHIP;
  }
  *graph_exec_out = exec;
  return DADD_OK;
}

int dadd_graph_launch(void* graph_exec, void* stream) {
  DADD_REQUIRE(graph_exec != nullptr, "graph_launch: null graph");
  DADD_HIP(hipGraphLaunch(static_cast<hipGraphExec_t>(graph_exec), static_cast<hipStream_t>(stream)));
  return DADD_OK;
}

int dadd_graph_destroy(void* graph_exec) {
  if (graph_exec) DADD_HIP(hipGraphExecDestroy(static_cast<hipGraphExec_t>(graph_exec)));
  return DADD_OK;
}

int dadd_prof_begin(void) {
  g_prof.rec.clear();
  g_prof.ms.clear();
  g_dadd_prof_on = 1;
  return DADD_OK;
}

int dadd_prof_end(int* n_records) {
  if (!g_dadd_prof_on) {
    dadd_set_error("prof_end without prof_begin");
    return DADD_ESTATE;
  }
  g_dadd_prof_on = 0;
  const size_t n = g_prof.rec.size();
  g_prof.ms.assign(n, 0.f);
  if (n > 0) DADD_HIP(hipEventSynchronize(g_prof.ev[2 * n - 1]));
  for (size_t i = 0; i < n; ++i) {
    DADD_HIP(hipEventSynchronize(g_prof.ev[2 * i + 1]));
    DADD_HIP(hipEventElapsedTime(&g_prof.ms[i], g_prof.ev[2 * i], g_prof.ev[2 * i + 1]));
  }
  if (n_records) *n_records = (int)n;
  return DADD_OK;
}

int dadd_prof_record(int i, const char** name, double out[3]) {
  DADD_REQUIRE(!g_dadd_prof_on && i >= 0 && (size_t)i < g_prof.ms.size() && name && out,
               "prof_record: index %d out of range (or profiling still active)", i);
  *name = g_prof.rec[i].name;
  out[0] = (double)g_prof.ms[i];
  out[1] = g_prof.rec[i].flop;
  out[2] = g_prof.rec[i].bytes;
  return DADD_OK;
}

}  // extern "C"
