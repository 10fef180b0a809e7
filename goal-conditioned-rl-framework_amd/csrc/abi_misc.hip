// abi_misc.hip — small C-ABI helpers: stand-alone sort op, hipEvent timing, raw device memory.
#include <cstdlib>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <string>

#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>

#include "common.h"
#include "gemm_mfma.h"
#include "her_bc.h"
#include "meet.h"
#include "ops.h"

// ---- host side of meet.h ---------------------------------------------------------------------------------------------------
namespace gcrl {
namespace {
int g_shared = -1;   // -1: not decided yet (GCRL_SHARED_GPU in the environment)
}
bool meet_device_shared() {
  if (g_shared < 0) {
    const char* e = std::getenv("GCRL_SHARED_GPU");
    g_shared = (e && *e && *e != '0') ? 1 : 0;
  }
  return g_shared == 1;
}
void meet_set_device_shared(bool on) { g_shared = on ? 1 : 0; }

// Is another PROCESS using this device through this library?  (the launch forms with in-kernel waits were switched off
// for ranks that share a GPU only under DataParallelUpdater; anyone else had to set GCRL_SHARED_GPU by hand.)  Every process that
// creates a handle on a device holds a SHARED advisory lock on a per-device presence file (named after the PCI bus id); whoever
// cannot convert it into an exclusive lock — non-blocking — is not alone, and from then on counts the device as shared.  Probed
// at handle creation and every few update calls (two system calls), so the process that was there first notices a later arrival
// too.  Not seen: a process with another /tmp, or another library on the same GPU (GCRL_SHARED_GPU=1 remains for those).
// GCRL_NO_DEVICE_LOCK=1 switches the probe off.
bool meet_probe_device(int device) {
  static std::map<int, int> fds;
  static const bool off = std::getenv("GCRL_NO_DEVICE_LOCK") != nullptr;
  if (off) return false;
  auto it = fds.find(device);
  if (it == fds.end()) {
    char bus[32] = {0};
    int fd = -2;
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) == hipSuccess && bus[0]) {
      for (char* c = bus; *c; ++c) if (*c == ':' || *c == '.') *c = '_';
      std::string path = std::string(std::getenv("TMPDIR") ? std::getenv("TMPDIR") : "/tmp") + "/gcrl_amd_gpu_" + bus + ".lock";
      fd = ::open(path.c_str(), O_RDWR | O_CREAT | O_CLOEXEC, 0666);
      if (fd >= 0) { (void)::fchmod(fd, 0666); (void)::flock(fd, LOCK_SH); } else fd = -2;
    } else {
      (void)hipGetLastError();
    }
    it = fds.emplace(device, fd).first;
  }
  if (it->second < 0) return false;
  if (::flock(it->second, LOCK_EX | LOCK_NB) == 0) {   // alone: back to the shared lock every process holds
    (void)::flock(it->second, LOCK_SH);
    return false;
  }
  (void)::flock(it->second, LOCK_SH);   // (a failed conversion drops the old lock on Linux: take it again)
  g_shared = 1;
  return true;
}

long long meet_capacity(const void* kernel, int threads, size_t lds_bytes) {
  if (meet_device_shared()) return 0;
  int dev = 0, cus = 0, per_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds_bytes) != hipSuccess) { (void)hipGetLastError(); return 0; }
  // LDS: the query divides 160 KB by the request, the hardware allocates in larger granules (32 256 B -> 4 resident, 31 744 B -> 5:
  // tools/occupancy_probe.hip) — recount with 1 KB granules and one granule held back
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, kernel) == hipSuccess) {
    const size_t lds = ((fa.sharedSizeBytes + lds_bytes + 1023) / 1024) * 1024;
    if (lds > 0) per_cu = std::min<long long>(per_cu, (long long)((160 * 1024 - 1024) / lds));
  }
  return (long long)cus * std::max(0, per_cu);
}
}  // namespace gcrl

namespace {
hipStream_t as_stream(void* s) {
  if (!s || s == GCRL_STREAM_LEGACY) return (hipStream_t) nullptr;
  return (hipStream_t)s;
}
__global__ __launch_bounds__(256) void hash_normal_fill_kernel(unsigned long long seed, unsigned long long ctr0, long long n, float* out) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    out[i] = gcrl::hash_normal(seed, ctr0 + (unsigned long long)i);
}
}  // namespace

extern "C" {

int gcrl_sort_truncate_mean(const float* in_dev, int64_t rows, int width, int drop, float* sorted_dev,
                            float* mean_dev, void* stream) {
  return gcrl::launch_sort_truncate_mean(as_stream(stream), in_dev, rows, width, drop, sorted_dev, mean_dev);
}

int gcrl_gemm_f32(const float* a, int64_t a_rs, int64_t a_cs, const float* b, int64_t b_rs, int64_t b_cs,
                  float* c, int64_t c_rs, const float* bias, int M, int N, int K, int act, int shape,
                  void* stream) {
  GCRL_CHECK_ARG(act >= 0 && act <= 3 && shape >= 0 && shape <= 5, "gcrl_gemm_f32: bad act/shape");
  gcrl::GemmDesc d;
  std::memset(&d, 0, sizeof(d));
  d.A = a; d.a_rs = a_rs; d.a_cs = a_cs;
  d.B = b; d.b_rs = b_rs; d.b_cs = b_cs;
  d.C = c; d.c_rs = c_rs;
  d.bias = bias;
  d.M = M; d.N = N; d.K = K;
  d.epi = act;
  return gcrl::launch_gemm_batch(as_stream(stream), &d, 1, shape);
}

int gcrl_gemm_dw_split_f32(const float* g, int64_t ldg, const float* x, int64_t ldx, float* dw, float* db, int out, int in, int batch,
                           int ksplit, float* sumsq, void* stream) {
  GCRL_CHECK_ARG(g && x && dw && db && out >= 1 && in >= 1 && batch >= 1 && ldg >= out && ldx >= in && ksplit >= 1 && ksplit <= 64,
                 "gcrl_gemm_dw_split_f32: bad arguments");
  hipStream_t st = as_stream(stream);
  const long long tiles = (long long)((out + 63) / 64) * ((in + 63) / 64);
  float *part = nullptr, *ss = nullptr;
  unsigned int* tick = nullptr;
  gcrl::GemmDesc d;
  std::memset(&d, 0, sizeof(d));
  d.A = g; d.a_rs = 1; d.a_cs = ldg;
  d.B = x; d.b_rs = ldx; d.b_cs = 1;
  d.C = dw; d.c_rs = in;
  d.M = out; d.N = in + 1; d.K = batch;
  d.ones_col = 1; d.col_out = db;
  d.ksplit = ksplit;
  int rc = GCRL_OK;
  auto cleanup = [&]() { (void)hipStreamSynchronize(st); if (part) (void)hipFree(part); if (tick) (void)hipFree(tick); if (ss) (void)hipFree(ss); };
  if (ksplit > 1) {
    GCRL_HIP(hipMalloc((void**)&part, (size_t)tiles * ksplit * gcrl::kTiledPartStride * sizeof(float)));
    if (hipMalloc((void**)&tick, (size_t)tiles * gcrl::kTicketStride * sizeof(unsigned int)) != hipSuccess ||
        hipMemsetAsync(tick, 0, (size_t)tiles * gcrl::kTicketStride * sizeof(unsigned int), st) != hipSuccess) { cleanup(); return gcrl::fail(GCRL_ERR_HIP, "gcrl_gemm_dw_split_f32: scratch"); }
    d.kpart = part; d.kticket = tick;
  }
  if (sumsq) {
    if (hipMalloc((void**)&ss, (size_t)tiles * 4 * sizeof(float)) != hipSuccess ||
        hipMemsetAsync(ss, 0, (size_t)tiles * 4 * sizeof(float), st) != hipSuccess) { cleanup(); return gcrl::fail(GCRL_ERR_HIP, "gcrl_gemm_dw_split_f32: scratch"); }
    d.sumsq_out = ss;
  }
  rc = gcrl::launch_gemm_batch(st, &d, 1, 4);
  if (!rc && ksplit > 1) rc = gcrl::launch_gemm_batch(st, &d, 1, 4);   // twice: the tickets must come back to zero by themselves
  if (!rc && sumsq) {
    std::vector<float> h((size_t)tiles * 4);
    if (hipMemcpyAsync(h.data(), ss, h.size() * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) rc = GCRL_ERR_HIP;
    float tot = 0.f;
    for (float v : h) tot += v;
    if (!rc && hipMemcpyAsync(sumsq, &tot, sizeof(float), hipMemcpyHostToDevice, st) != hipSuccess) rc = GCRL_ERR_HIP;
  }
  cleanup();
  return rc;
}

// The whole problem record, up to kMaxProb problems per call (include/gcrl.h).  Operands are assumed below 2 GiB each: the kernels'
// 32-bit byte offsets (gemm_mfma.h, gemm_tiled.h) cannot be reached at test sizes and are not checked here.
int gcrl_gemm_batch_f32(gcrl_gemm_problem* p, int n, int shape, void* stream) {
  GCRL_CHECK_ARG(shape >= 0 && shape <= 5, "gcrl_gemm_batch_f32: bad shape %d", shape);
  hipStream_t st = as_stream(stream);
  if (n < 1 || n > gcrl::kMaxProb) return gcrl::launch_gemm_batch(st, nullptr, n, shape);   // (the launcher's own refusal)
  GCRL_CHECK_ARG(p, "gcrl_gemm_batch_f32: null problem array");
  struct Scratch {   // freed, after the stream has drained, when the call returns
    hipStream_t st;
    std::vector<void*> mem;
    ~Scratch() {
      if (mem.empty()) return;
      (void)hipStreamSynchronize(st);
      for (void* m : mem) (void)hipFree(m);
    }
    void* zeroed(size_t bytes, bool zero) {
      void* m = nullptr;
      if (hipMalloc(&m, bytes) != hipSuccess) return nullptr;
      mem.push_back(m);
      if (zero && hipMemsetAsync(m, 0, bytes, st) != hipSuccess) return nullptr;
      return m;
    }
  } sc{st, {}};
  gcrl::GemmDesc d[gcrl::kMaxProb];
  int form[gcrl::kMaxProb], nss[gcrl::kMaxProb];
  bool twice = false;
  for (int i = 0; i < n; ++i) {
    const gcrl_gemm_problem& q = p[i];
    GCRL_CHECK_ARG(q.act >= 0 && q.act <= 3 && q.mul >= 0 && q.mul <= 3 && q.shape_hint >= 0 && q.shape_hint <= 5 && q.ksplit >= 0 && q.ksplit <= 64,
                   "gcrl_gemm_batch_f32: problem %d: bad act=%d / mul=%d / shape_hint=%d / ksplit=%d", i, q.act, q.mul, q.shape_hint, q.ksplit);
    GCRL_CHECK_ARG(q.mul == 0 || q.h_dev, "gcrl_gemm_batch_f32: problem %d: mul=%d needs the saved activations", i, q.mul);
    gcrl::GemmDesc& g = d[i];
    std::memset(&g, 0, sizeof(g));
    g.A = q.a_dev; g.a_rs = q.a_rs; g.a_cs = q.a_cs;
    g.B = q.b_dev; g.b_rs = q.b_rs; g.b_cs = q.b_cs;
    g.C = q.c_dev; g.c_rs = q.c_rs;
    g.bias = q.bias_dev;
    g.H = q.h_dev; g.h_rs = q.h_rs;
    g.col_out = q.col_out_dev;
    g.M = q.M; g.N = q.N; g.K = q.K;
    g.epi = q.act; g.mul = q.mul; g.ones_col = q.ones_col ? 1 : 0;
    g.slot = q.slot_dev; g.a_slot = q.a_slot; g.b_slot = q.b_slot; g.c_slot = q.c_slot; g.h_slot = q.h_slot;
    g.shape_hint = q.shape_hint; g.ksplit = q.ksplit;
    g.bn_part = q.bn_part_dev;
    g.sumsq_out = q.sumsq_dev;   // (non-null is all the form rule reads; the partial array replaces it below)
    form[i] = shape ? shape : (g.shape_hint ? g.shape_hint : gcrl::gemm_shape_of(g));
    p[i].form_out = form[i];
    nss[i] = 0;
    if (g.M < 1 || g.N < 1 || g.K < 1) continue;   // (refused by the launcher: nothing to size)
    if (g.ksplit > 1) {
      const size_t tiles = (size_t)((g.M + 63) / 64) * (size_t)((g.N - g.ones_col + 63) / 64 > 0 ? (g.N - g.ones_col + 63) / 64 : 1);
      g.kpart = (float*)sc.zeroed(tiles * g.ksplit * gcrl::kTiledPartStride * sizeof(float), false);
      g.kticket = (unsigned int*)sc.zeroed(tiles * gcrl::kTicketStride * sizeof(unsigned int), true);
      if (!g.kpart || !g.kticket) return gcrl::fail(GCRL_ERR_HIP, "gcrl_gemm_batch_f32: problem %d: scratch", i);
      if (form[i] == 4) twice = true;
    }
    if (q.sumsq_dev) {
      nss[i] = std::max(0, gcrl::gemm_sumsq_partials(g, form[i]));
      g.sumsq_out = (float*)sc.zeroed((size_t)std::max(nss[i], 1) * sizeof(float), true);
      if (!g.sumsq_out) return gcrl::fail(GCRL_ERR_HIP, "gcrl_gemm_batch_f32: problem %d: scratch", i);
    }
  }
  if (int rc = gcrl::launch_gemm_batch(st, d, n, shape)) return rc;
  if (twice) {   // again: the tickets must have come back to zero by themselves; what a split problem wrote is "not written" before
    for (int i = 0; i < n; ++i) {
      const gcrl::GemmDesc& g = d[i];
      if (!(g.ksplit > 1 && form[i] == 4)) continue;
      int s = 0;
      if (g.slot) {
        GCRL_HIP(hipMemcpyAsync(&s, g.slot, sizeof(int), hipMemcpyDeviceToHost, st));
        GCRL_HIP(hipStreamSynchronize(st));
      }
      const int cols = g.N - g.ones_col;
      if (cols >= 1 && g.c_rs >= cols)
        GCRL_HIP(hipMemset2DAsync(g.C + (long long)s * g.c_slot, (size_t)g.c_rs * sizeof(float), 0xff, (size_t)cols * sizeof(float), (size_t)g.M, st));
      if (g.ones_col) GCRL_HIP(hipMemsetAsync(g.col_out, 0xff, (size_t)g.M * sizeof(float), st));
      if (nss[i]) GCRL_HIP(hipMemsetAsync(g.sumsq_out, 0, (size_t)nss[i] * sizeof(float), st));
    }
    if (int rc = gcrl::launch_gemm_batch(st, d, n, shape)) return rc;
  }
  for (int i = 0; i < n; ++i) {
    if (!p[i].sumsq_dev) continue;
    std::vector<float> h((size_t)nss[i]);
    if (nss[i]) GCRL_HIP(hipMemcpyAsync(h.data(), d[i].sumsq_out, h.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    GCRL_HIP(hipStreamSynchronize(st));
    float tot = 0.f;
    for (float v : h) tot += v;   // index order
    GCRL_HIP(hipMemcpyAsync(p[i].sumsq_dev, &tot, sizeof(float), hipMemcpyHostToDevice, st));
    GCRL_HIP(hipStreamSynchronize(st));   // (tot is on this stack)
  }
  GCRL_HIP(hipStreamSynchronize(st));
  return GCRL_OK;
}

int gcrl_bn_relu_fwd_f32(const float* z, int B, int H, const float* gamma, const float* beta, float* h, float* xhat, float* invstd,
                         float* running_mean, float* running_var, float* scratch, void* stream) {
  GCRL_CHECK_ARG(z && gamma && beta && h && running_mean && running_var && scratch && B >= 1 && H >= 4, "gcrl_bn_relu_fwd_f32: bad arguments");
  return gcrl::launch_bn_relu_fwd(as_stream(stream), z, B, H, gamma, beta, h, xhat, invstd, running_mean, running_var, scratch);
}

int gcrl_bn_relu_bwd_f32(const float* dh, const float* xhat, const float* invstd, const float* gamma, const float* beta, int B, int H,
                         float* dz, float* dgamma, float* dbeta, float* scratch, void* stream) {
  GCRL_CHECK_ARG(dh && xhat && invstd && gamma && beta && dz && dgamma && dbeta && scratch && B >= 1 && H >= 4,
                 "gcrl_bn_relu_bwd_f32: bad arguments");
  return gcrl::launch_bn_relu_bwd(as_stream(stream), dh, nullptr, xhat, invstd, gamma, beta, B, H, dz, dgamma, dbeta, scratch);
}

// row-group exchange scratch of the stand-alone slab entries (allocated on first use, process lifetime: test entry points)
static int slab_scratch(int H, float** xchg, unsigned int** bar) {
  static float* x = nullptr; static unsigned int* b = nullptr; static int cap = 0;
  if (H > cap) {
    GCRL_HIP(hipDeviceSynchronize());
    if (x) (void)hipFree(x);
    if (b) (void)hipFree(b);
    GCRL_HIP(hipMalloc((void**)&x, (size_t)gcrl::bn_slab_xchg_floats(H) * sizeof(float)));
    GCRL_HIP(hipMalloc((void**)&b, (size_t)gcrl::bn_slab_bar_words(H) * sizeof(unsigned int)));
    GCRL_HIP(hipMemset(b, 0, (size_t)gcrl::bn_slab_bar_words(H) * sizeof(unsigned int)));
    GCRL_HIP(hipDeviceSynchronize());
    cap = H;
  }
  *xchg = x; *bar = b;
  return GCRL_OK;
}
// The meeting counters are monotonic and must be a multiple of a launch's row-group count when it starts (meet.h): an agent's
// own counters always are (its row-group count never changes); this process-wide scratch serves launches of ANY shape, so
// every launch starts from zeroed counters (stream-ordered)
static int slab_scratch_reset(int H, float* xchg, unsigned int* bar, hipStream_t st) { return gcrl::bn_slab_scratch_reset(xchg, bar, H, st); }

int gcrl_bn_linear_slab_fwd_f32(const float* x, int64_t ldx, const float* w, const float* bias, const float* gamma, const float* beta,
                                int B, int H, int K, float* h, float* xhat, float* invstd, float* bstat, int row_split, void* stream) {
  GCRL_CHECK_ARG(x && w && bias && gamma && beta && h && bstat && K >= 1 && ldx >= K && gcrl::bn_slab_ok(B, H),
                 "gcrl_bn_linear_slab_fwd_f32: bad arguments (B <= 512, H a multiple of 16)");
  gcrl::BnSlabFwd f;
  std::memset(&f, 0, sizeof(f));
  f.n = 1;
  f.p[0] = gcrl::BnSlabFwdProb{x, 0, h, xhat, invstd, bstat};
  f.W = w; f.bias = bias; f.gamma = gamma; f.beta = beta; f.ldx = ldx; f.B = B; f.H = H; f.K = K;
  if (row_split > 1) {
    f.rsplit = row_split;
    if (int rc = slab_scratch(H, &f.xchg, &f.bar)) return rc;
    if (int rc = slab_scratch_reset(H, f.xchg, f.bar, as_stream(stream))) return rc;
  }
  return gcrl::launch_bn_linear_fwd_slab(as_stream(stream), f);
}

int gcrl_bn_linear_slab_bwd_f32(const float* g_up, int64_t ldg, int K_up, const float* w_up, float* xhat_dz, const float* invstd,
                                const float* gamma, const float* beta, int B, int H, float* dgamma, float* dbeta, int row_split, void* stream) {
  GCRL_CHECK_ARG(g_up && w_up && xhat_dz && invstd && gamma && beta && dgamma && dbeta && K_up >= 1 && ldg >= K_up && gcrl::bn_slab_ok(B, H),
                 "gcrl_bn_linear_slab_bwd_f32: bad arguments (B <= 512, H a multiple of 16)");
  gcrl::BnSlabBwd b;
  std::memset(&b, 0, sizeof(b));
  b.nup = 1;
  b.G[0] = g_up; b.ldg[0] = ldg; b.K[0] = K_up; b.W[0] = w_up; b.ldw[0] = H;
  b.xhat_dz = xhat_dz; b.invstd = invstd; b.gamma = gamma; b.beta = beta; b.dgamma = dgamma; b.dbeta = dbeta;
  b.B = B; b.H = H;
  if (row_split > 1) {
    b.rsplit = row_split;
    if (int rc = slab_scratch(H, &b.xchg, &b.bar)) return rc;
    if (int rc = slab_scratch_reset(H, b.xchg, b.bar, as_stream(stream))) return rc;
  }
  return gcrl::launch_bn_linear_bwd_slab(as_stream(stream), b);
}

}  // extern "C"

// ---- the stage kernels as single problems (test entry points) -----------------------------------------------------------
namespace {
// Device scratch of one call: the control record every stage kernel reads (zeroed: batch slot 0, metrics slot 0) with
// `do_alpha`, the device scalars log_alpha / alpha, a zeroed ticket word on its own line, `part_floats` floats of partial sums.
// Freed, after the stream has drained, when the call returns.
struct StageScratch {
  static constexpr size_t kScalars = 64, kTicket = 128, kPart = 256;
  static_assert(sizeof(gcrl::StepCtrl) <= kScalars, "control record");
  char* base = nullptr;
  hipStream_t st = nullptr;
  ~StageScratch() {
    if (!base) return;
    (void)hipStreamSynchronize(st);
    (void)hipFree(base);
  }
  int init(hipStream_t stream, int do_alpha, float log_alpha, float alpha, size_t part_floats, int batch_slot = 0) {
    st = stream;
    GCRL_HIP(hipMalloc((void**)&base, kPart + part_floats * sizeof(float)));
    char img[kPart];
    std::memset(img, 0, sizeof(img));
    gcrl::StepCtrl c;
    std::memset(&c, 0, sizeof(c));
    c.do_alpha = do_alpha;
    c.batch_slot = batch_slot;
    std::memcpy(img, &c, sizeof(c));
    const float sc[2] = {log_alpha, alpha};
    std::memcpy(img + kScalars, sc, sizeof(sc));
    GCRL_HIP(hipMemcpyAsync(base, img, sizeof(img), hipMemcpyHostToDevice, st));
    GCRL_HIP(hipStreamSynchronize(st));   // (img is on this stack)
    return GCRL_OK;
  }
  const gcrl::StepCtrl* ctrl() const { return reinterpret_cast<const gcrl::StepCtrl*>(base); }
  float* log_alpha() const { return reinterpret_cast<float*>(base + kScalars); }
  float* alpha() const { return reinterpret_cast<float*>(base + kScalars) + 1; }
  unsigned int* ticket() const { return reinterpret_cast<unsigned int*>(base + kTicket); }
  float* part() const { return reinterpret_cast<float*>(base + kPart); }
};
// "not written" before a repeated launch: all-ones words (NaN as fp32)
int stage_poison(hipStream_t st, float* p, size_t n) {
  if (p) GCRL_HIP(hipMemsetAsync(p, 0xff, n * sizeof(float), st));
  return GCRL_OK;
}
}  // namespace

extern "C" {

int gcrl_td_loss_f32(const float* r, const float* d, const float* qt, const float* q, const float* logp_next, float alpha, const float* w,
                     int B, int C, int drop, int target_kind, int loss_kind, float gamma, float clamp_lo, int multi_block, float* dq,
                     float* td_abs, float* metrics, void* stream) {
  GCRL_CHECK_ARG(r && d && qt && q && dq && metrics && B >= 1 && B <= (1 << 24) && C >= 1 && C <= gcrl::kMaxCritics,
                 "gcrl_td_loss_f32: bad arguments (B=%d C=%d)", B, C);
  GCRL_CHECK_ARG(target_kind >= gcrl::TGT_DDPG && target_kind <= gcrl::TGT_TRUNC_ENT && (loss_kind == gcrl::LOSS_MSE || loss_kind == gcrl::LOSS_SMOOTH_L1),
                 "gcrl_td_loss_f32: bad target kind %d / loss kind %d", target_kind, loss_kind);
  GCRL_CHECK_ARG(target_kind == gcrl::TGT_TRUNC_ENT ? (drop >= 0 && drop < C) : drop == 0, "gcrl_td_loss_f32: bad drop=%d (C=%d)", drop, C);
  GCRL_CHECK_ARG(target_kind == gcrl::TGT_DDPG ? C == 1 : (target_kind == gcrl::TGT_TRUNC_ENT || C == 2),
                 "gcrl_td_loss_f32: target kind %d with C=%d", target_kind, C);
  GCRL_CHECK_ARG((target_kind == gcrl::TGT_MIN_ENT || target_kind == gcrl::TGT_TRUNC_ENT) ? logp_next != nullptr : true,
                 "gcrl_td_loss_f32: the entropy targets need logp_next");
  GCRL_CHECK_ARG(multi_block >= 0 && multi_block <= 4 && (multi_block == 0 || B >= 1024),
                 "gcrl_td_loss_f32: bad multi_block=%d (the multi-workgroup form starts at B = 1024)", multi_block);
  hipStream_t st = as_stream(stream);
  StageScratch s;
  if (int rc = s.init(st, 0, 0.f, 0.f, multi_block ? (size_t)64 * ((B + 255) / 256) : 0)) return rc;
  gcrl::TdLossArgs a;
  std::memset(&a, 0, sizeof(a));
  a.cur = s.ctrl();
  a.r = r; a.d = d; a.qt = qt; a.q = q; a.logp_next = logp_next; a.alpha_const = alpha; a.dq = dq; a.w = w; a.td_abs = td_abs;
  a.metrics = metrics;
  a.B = B; a.C = C; a.drop = drop; a.target_kind = target_kind; a.loss_kind = loss_kind; a.gamma = gamma; a.clamp_lo = clamp_lo;
  if (multi_block) { a.part = s.part(); a.ticket = s.ticket(); }
  int rc = gcrl::launch_td_loss(st, a);
  for (int i = 1; !rc && i < multi_block; ++i) {   // again: the ticket must have come back to zero by itself
    if ((rc = stage_poison(st, dq, (size_t)C * B)) || (rc = stage_poison(st, td_abs, (size_t)B)) ||
        (rc = stage_poison(st, metrics, gcrl::kMetricFloats))) break;
    rc = gcrl::launch_td_loss(st, a);
  }
  return rc;
}

int gcrl_bc_qfilter_f32(const float* spa, const float* sa, int ldx, int col0, int slots, int slot, const float* q_pi, const float* q_a, int B, int Bd,
                        int A, double bc_weight, float* dact, int ld_dact, float* mask, float* metrics, void* stream) {
  GCRL_CHECK_ARG(spa && sa && q_pi && dact && metrics, "gcrl_bc_qfilter_f32: null argument");
  GCRL_CHECK_ARG(slots >= 1 && slot >= 0 && slot < slots, "gcrl_bc_qfilter_f32: batch slot %d of %d", slot, slots);
  GCRL_CHECK_ARG(std::isfinite(bc_weight) && bc_weight > 0.0, "gcrl_bc_qfilter_f32: bc_weight: %g is not a finite weight > 0", bc_weight);
  hipStream_t st = as_stream(stream);
  gcrl::BcArgs a;
  std::memset(&a, 0, sizeof(a));
  a.spa = spa; a.sa = sa; a.slot_x = (long long)B * ldx; a.ldx = ldx; a.col0 = col0;
  a.q_pi = q_pi; a.q_a = q_a; a.dact = dact; a.ld_dact = ld_dact; a.mask = mask; a.metrics = metrics;
  a.B = B; a.Bd = Bd; a.A = A;
  a.c = (float)((2.0 * bc_weight) / (double)Bd); a.w_bd = (float)(bc_weight / (double)Bd);
  a.cur = reinterpret_cast<const gcrl::StepCtrl*>(metrics);   // (any non-null value: checked below, replaced once the scratch exists)
  GCRL_CHECK_ARG(gcrl::bc_args_ok(a), "gcrl_bc_qfilter_f32: bad arguments (B=%d Bd=%d A=%d ldx=%d col0=%d ld_dact=%d)", B, Bd, A, ldx, col0, ld_dact);
  StageScratch s;
  if (int rc = s.init(st, 0, 0.f, 0.f, 0, slot)) return rc;
  a.cur = s.ctrl();
  return gcrl::launch_bc_qfilter(st, a);
}

int gcrl_tanh_gauss_fwd_f32(const float* mu, const float* ls_raw, int ld_head, const float* eps, int B, int A, int deterministic,
                            float* act, int ld_act, float* logp, float* save_eps, float* save_std, void* stream) {
  GCRL_CHECK_ARG(mu && act && B >= 1 && A >= 1 && ld_head >= A && ld_act >= A && (long long)B * std::max(ld_head, ld_act) < (1ll << 31),
                 "gcrl_tanh_gauss_fwd_f32: bad arguments (B=%d A=%d ld_head=%d ld_act=%d)", B, A, ld_head, ld_act);
  GCRL_CHECK_ARG(deterministic || (ls_raw && eps && logp), "gcrl_tanh_gauss_fwd_f32: sampling needs ls_raw, eps and logp");
  GCRL_CHECK_ARG((save_eps == nullptr) == (save_std == nullptr), "gcrl_tanh_gauss_fwd_f32: save_eps and save_std go together");
  hipStream_t st = as_stream(stream);
  StageScratch s;
  if (int rc = s.init(st, 0, 0.f, 0.f, 0)) return rc;
  gcrl::TanhGaussArgs a;
  std::memset(&a, 0, sizeof(a));
  a.cur = s.ctrl();
  a.mu = mu; a.ls_raw = ls_raw; a.ld_head = ld_head; a.eps = eps;
  a.act = act; a.ld_act = ld_act; a.logp = logp; a.save_eps = save_eps; a.save_std = save_std;
  a.B = B; a.A = A; a.deterministic = deterministic ? 1 : 0;
  return gcrl::launch_tanh_gauss_fwd(st, a);   // (run.layers = 0: no running-statistics rider)
}

int gcrl_tanh_gauss_bwd_f32(const float* dact, int C, int ld_dact, const float* act, int ld_act, const float* eps, const float* std_dev,
                            const float* ls_raw, int ld_head, float alpha, int B, int A, float* gmu, float* gls, int ld_g, void* stream) {
  GCRL_CHECK_ARG(dact && act && eps && std_dev && ls_raw && gmu && gls && B >= 1 && A >= 1 && C >= 1 && C <= gcrl::kMaxCritics &&
                 ld_dact >= A && ld_act >= A && ld_head >= A && ld_g >= A &&
                 (long long)B * std::max(std::max(ld_dact, ld_act), std::max(ld_head, ld_g)) < (1ll << 31),
                 "gcrl_tanh_gauss_bwd_f32: bad arguments (B=%d A=%d C=%d)", B, A, C);
  hipStream_t st = as_stream(stream);
  StageScratch s;
  if (int rc = s.init(st, 0, 0.f, 0.f, 0)) return rc;
  gcrl::TanhGaussBwdArgs a;
  std::memset(&a, 0, sizeof(a));
  a.dact = dact; a.C = C; a.ld_dact = ld_dact; a.dact_stride = (long long)B * ld_dact;
  a.act = act; a.ld_act = ld_act; a.cur = s.ctrl();
  a.eps = eps; a.std = std_dev; a.ls_raw = ls_raw; a.ld_head = ld_head;
  a.alpha_const = alpha;
  a.gmu = gmu; a.gls = gls; a.ld_g = ld_g;
  a.B = B; a.A = A;
  return gcrl::launch_tanh_gauss_bwd(st, a);
}

int gcrl_actor_select_f32(const float* q, const float* logp, float alpha, int B, int C, int drop, int min_of_two, int do_alpha,
                          float target_entropy, float log_alpha, int form, float* dq, float* metrics, float* grad_log_alpha, void* stream) {
  GCRL_CHECK_ARG(q && logp && dq && metrics && B >= 1 && B <= (1 << 24) && C >= 1 && C <= gcrl::kMaxCritics && drop >= 0 && drop < C,
                 "gcrl_actor_select_f32: bad arguments (B=%d C=%d drop=%d)", B, C, drop);
  GCRL_CHECK_ARG(!min_of_two || (C == 2 && drop == 0), "gcrl_actor_select_f32: min_of_two needs C = 2, drop = 0 (C=%d drop=%d)", C, drop);
  GCRL_CHECK_ARG(form >= 0 && form <= 3 && (form == 0 || grad_log_alpha) && (form < 2 || B >= 1024),
                 "gcrl_actor_select_f32: bad form=%d (1..3 need grad_log_alpha; the multi-workgroup form starts at B = 1024)", form);
  hipStream_t st = as_stream(stream);
  StageScratch s;
  if (int rc = s.init(st, do_alpha ? 1 : 0, log_alpha, alpha, form >= 2 ? (size_t)8 * ((B + 255) / 256) : 0)) return rc;
  gcrl::ActorSelArgs a;
  std::memset(&a, 0, sizeof(a));
  a.cur = s.ctrl();
  a.q = q; a.logp = logp; a.dq = dq; a.metrics = metrics;
  a.B = B; a.C = C; a.drop = drop; a.min2 = min_of_two ? 1 : 0;
  if (form == 0) {
    a.alpha_const = alpha;
    return gcrl::launch_actor_select(st, a);
  }
  a.alpha_dev = s.alpha();
  a.mean_x = q; a.mean_n = C * B; a.mean_index = gcrl::MET_Q;   // the rider: mean of the critics' outputs
  if (form >= 2) { a.part = s.part(); a.ticket = s.ticket(); }
  gcrl::AlphaArgs al;
  std::memset(&al, 0, sizeof(al));
  al.cur = s.ctrl();
  al.logp = logp; al.B = B; al.target_entropy = target_entropy;
  al.log_alpha = s.log_alpha(); al.alpha = s.alpha(); al.grad_out = grad_log_alpha;
  al.metrics = metrics;
  al.phase = 0;
  int rc = gcrl::launch_actor_select_alpha(st, a, al);
  if (!rc && form == 2) {   // again: the ticket must have come back to zero by itself
    if ((rc = stage_poison(st, dq, (size_t)C * B)) || (rc = stage_poison(st, metrics, gcrl::kMetricFloats)) ||
        (rc = stage_poison(st, do_alpha ? grad_log_alpha : nullptr, 1))) return rc;   // (no gradient is written without do_alpha)
    rc = gcrl::launch_actor_select_alpha(st, a, al);
  }
  return rc;
}

int gcrl_quantile_td_f32(const float* r, const float* d, const float* zt, const float* z, const float* logp_next, float alpha, int B, int C,
                         int Q, int drop, float gamma, float* y, float* dz, float* row_loss, float* row_td, float* metrics, void* stream) {
  GCRL_CHECK_ARG(r && d && zt && z && logp_next && y && dz && row_loss && row_td && metrics && B >= 1 && B <= (1 << 24),
                 "gcrl_quantile_td_f32: bad arguments (B=%d)", B);
  hipStream_t st = as_stream(stream);
  StageScratch s;
  if (int rc = s.init(st, 0, 0.f, alpha, 0)) return rc;
  gcrl::QuantileArgs a;
  std::memset(&a, 0, sizeof(a));
  a.cur = s.ctrl();
  a.r = r; a.d = d; a.zt = zt; a.z = z; a.logp_next = logp_next; a.alpha_dev = s.alpha();
  a.y = y; a.dz = dz; a.row_loss = row_loss; a.row_td = row_td; a.metrics = metrics;
  a.B = B; a.C = C; a.Q = Q; a.drop = drop; a.gamma = gamma;
  return gcrl::launch_quantile_td(st, a);   // (C, Q, drop: the launcher's own refusal)
}

int gcrl_quantile_actor_f32(const float* z, const float* logp, float alpha, int B, int C, int Q, float* dz, float* metrics, void* stream) {
  GCRL_CHECK_ARG(z && logp && dz && metrics && B >= 1 && B <= (1 << 24) && C >= 1 && C <= gcrl::kMaxCritics && Q >= 1 && C * Q <= 64,
                 "gcrl_quantile_actor_f32: bad arguments (B=%d C=%d Q=%d)", B, C, Q);
  hipStream_t st = as_stream(stream);
  StageScratch s;
  if (int rc = s.init(st, 0, 0.f, alpha, 0)) return rc;
  gcrl::QuantileActorArgs a{s.ctrl(), z, logp, s.alpha(), dz, metrics, B, C, Q};
  return gcrl::launch_quantile_actor(st, a);
}

int gcrl_td3_smooth_f32(float* act, int ld, int B, int A, const float* eps, float policy_noise, float noise_clip, void* stream) {
  GCRL_CHECK_ARG(act && eps && B >= 1 && A >= 1 && ld >= A && (long long)B * ld < (1ll << 31) && noise_clip >= 0.f,
                 "gcrl_td3_smooth_f32: bad arguments (B=%d A=%d ld=%d)", B, A, ld);
  hipStream_t st = as_stream(stream);
  StageScratch s;
  if (int rc = s.init(st, 0, 0.f, 0.f, 0)) return rc;
  return gcrl::launch_td3_smooth(st, s.ctrl(), act, 0, ld, B, A, eps, policy_noise, noise_clip, 0ull);
}

int gcrl_set_shared_device(int shared) {
  gcrl::meet_set_device_shared(shared != 0);
  return GCRL_OK;
}

int gcrl_hash_normal_fill(uint64_t seed, uint64_t ctr0, int64_t n, float* out_dev, void* stream) {
  GCRL_CHECK_ARG(out_dev && n >= 1, "gcrl_hash_normal_fill: bad arguments");
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(hash_normal_fill_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), (unsigned long long)seed,
                     (unsigned long long)ctr0, (long long)n, out_dev);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

void* gcrl_event_create(void) {
  hipEvent_t ev = nullptr;
  if (hipEventCreate(&ev) != hipSuccess) { gcrl::fail(GCRL_ERR_HIP, "hipEventCreate failed"); return nullptr; }
  return (void*)ev;
}
void gcrl_event_destroy(void* ev) { if (ev) (void)hipEventDestroy((hipEvent_t)ev); }
int gcrl_event_record(void* ev, void* stream) {
  GCRL_CHECK_ARG(ev, "gcrl_event_record: null event");
  GCRL_HIP(hipEventRecord((hipEvent_t)ev, as_stream(stream)));
  return GCRL_OK;
}
int gcrl_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms_out) {
  GCRL_CHECK_ARG(ev_start && ev_stop && ms_out, "gcrl_event_elapsed_ms: null argument");
  GCRL_HIP(hipEventSynchronize((hipEvent_t)ev_stop));
  GCRL_HIP(hipEventElapsedTime(ms_out, (hipEvent_t)ev_start, (hipEvent_t)ev_stop));
  return GCRL_OK;
}
int gcrl_stream_synchronize(void* stream) {
  GCRL_HIP(hipStreamSynchronize(as_stream(stream)));
  return GCRL_OK;
}
void* gcrl_malloc(size_t bytes) {
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) { gcrl::fail(GCRL_ERR_HIP, "hipMalloc(%zu) failed", bytes); return nullptr; }
  return p;
}
void gcrl_free(void* p) { if (p) (void)hipFree(p); }
int gcrl_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream) {
  GCRL_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, as_stream(stream)));
  GCRL_HIP(hipStreamSynchronize(as_stream(stream)));
  return GCRL_OK;
}
int gcrl_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream) {
  GCRL_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, as_stream(stream)));
  GCRL_HIP(hipStreamSynchronize(as_stream(stream)));
  return GCRL_OK;
}

}  // extern "C"
