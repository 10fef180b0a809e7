// her_norm.hip — sample-time observation and goal normalisation of a HER ring (normalize = "sample").
//
// A ring in GCRL_NORMALIZE_SAMPLE holds RAW [obs | dg] states, raw next states and raw achieved goals; what leaves it is normalised
// with the statistics as they stand in stream order when the batch is gathered, not with those of the moment of the push.  Two
// things live here:
//   her_norm_rows_kernel / her_norm_dense_kernel   ONE in-place pass behind a gather launch over the batch it wrote: column c < D of
//       s and ns becomes norm_apply(x, mean_o[c], norm_den(var_o[c]), clip_o), column D <= c < S the same with the goal normaliser
//       — bit for bit what gcrl_normalizer_normalize returns for those columns (norm_math.h is shared).  Actions, rewards, done
//       flags and padding columns keep their bit patterns.  One kernel serves every gather family, form and index source: it is a
//       launch of its own behind them, once per gather, not a stage of theirs.
//   her_process_step_raw_*_kernel   siblings of her_ring.hip's fused process_step launch: the same two statistics updates by the same
//       norm_update_col calls, then the step's rows and achieved goals staged as they came.
// The rule is restated in numpy in tests/her_normalize_ref.py, which is its definition.
//
// A translation unit of its own: every other unit's kernels keep their code, byte for byte.  No kernel here waits for another
// workgroup, uses atomics or per-thread scratch.
#include "her_ring.h"
#include "norm_math.h"
#include "per_tree.h"

namespace {

constexpr int kMaxS = 136;     // state columns: obs_dim <= 128, goal_dim <= 8
constexpr int kMaxG = 8;
constexpr int kRows = 64;      // rows of one workgroup
constexpr int kPayW = 32;      // her_ring.hip's per-env payload [t | r | d | a(A) | ag(G)]

struct NormArgs {
  float* x0; float* x1; float* x2;   // the matrices of one gather: sa, nsa, spa (rows) / out_s, out_ns (dense); blockIdx.y picks
  int ld0, ld1, ld2;                 // their row strides in floats
  long long n;                       // rows
  int D, S;                          // a state is [obs (D) | goal (S - D)]
  int lo, hi;                        // the columns that are normalised: [lo, hi) with lo in {0, D}, hi in {D, S}
  const double* mean; const double* var; double clip; int mode;       // observation normaliser (null: columns [0, D) stay raw)
  const double* gmean; const double* gvar; double gclip; int gmode;   // goal normaliser (null: columns [D, S) stay raw)
};

// (mean, den) of the normalised columns, once per workgroup: one norm_den per column, not one per element
__device__ inline void load_stats(const NormArgs& p, double* s_mean, double* s_den) {
  for (int c = p.lo + (int)threadIdx.x; c < p.hi; c += (int)blockDim.x) {
    if (c < p.D) { s_mean[c] = p.mean[c]; s_den[c] = gcrl::norm_den(p.var[c], (p.mode & gcrl::NORM_F32) != 0); }
    else { s_mean[c] = p.gmean[c - p.D]; s_den[c] = gcrl::norm_den(p.gvar[c - p.D], (p.gmode & gcrl::NORM_F32) != 0); }
  }
  __syncthreads();
}

__device__ inline float apply_col(const NormArgs& p, const double* s_mean, const double* s_den, int c, float x) {
  if (c < p.lo || c >= p.hi) return x;
  if (c < p.D) return gcrl::norm_apply(x, s_mean[c], s_den[c], p.clip, gcrl::norm_apply_f32(p.mode));
  return gcrl::norm_apply(x, s_mean[c], s_den[c], p.gclip, gcrl::norm_apply_f32(p.gmode));
}

// Rows of stride ld (a multiple of 4 floats, 16-byte aligned base): a thread owns 16-byte quads — one load, up to four norm_apply,
// one store.  A quad that straddles lo or hi writes its other components back as it read them.  Workgroup (bx, m): rows
// [64 bx, 64 bx + 64) of matrix m, the last one partial.  Every address lies inside row r < n at columns < roundup(hi, 4) <= ld.
__global__ __launch_bounds__(256) void her_norm_rows_kernel(NormArgs p) {
  __shared__ double s_mean[kMaxS], s_den[kMaxS];
  load_stats(p, s_mean, s_den);
  float* x = blockIdx.y == 0 ? p.x0 : (blockIdx.y == 1 ? p.x1 : p.x2);
  const int ld = blockIdx.y == 0 ? p.ld0 : (blockIdx.y == 1 ? p.ld1 : p.ld2);
  const int q0 = p.lo >> 2, nq = ((p.hi + 3) >> 2) - q0;
  const long long row0 = (long long)blockIdx.x * kRows;
  const int rows = (int)(p.n - row0 < kRows ? p.n - row0 : kRows);
  for (int t = threadIdx.x; t < rows * nq; t += 256) {
    const int r = t / nq, c = 4 * (q0 + (t - r * nq));
    float4* at = reinterpret_cast<float4*>(x + (row0 + r) * ld + c);
    float4 v = *at;
    v.x = apply_col(p, s_mean, s_den, c, v.x);
    v.y = apply_col(p, s_mean, s_den, c + 1, v.y);
    v.z = apply_col(p, s_mean, s_den, c + 2, v.z);
    v.w = apply_col(p, s_mean, s_den, c + 3, v.w);
    *at = v;
  }
}

// The public sample()'s dense outputs and a caller's own matrices: any leading dimension and alignment, one element per load and store.
__global__ __launch_bounds__(256) void her_norm_dense_kernel(NormArgs p) {
  __shared__ double s_mean[kMaxS], s_den[kMaxS];
  load_stats(p, s_mean, s_den);
  float* x = blockIdx.y == 0 ? p.x0 : (blockIdx.y == 1 ? p.x1 : p.x2);
  const int ld = blockIdx.y == 0 ? p.ld0 : (blockIdx.y == 1 ? p.ld1 : p.ld2);
  const int w = p.hi - p.lo;
  const long long row0 = (long long)blockIdx.x * kRows;
  const int rows = (int)(p.n - row0 < kRows ? p.n - row0 : kRows);
  for (int t = threadIdx.x; t < rows * w; t += 256) {
    const int r = t / w, c = p.lo + (t - r * w);
    float* at = x + (row0 + r) * ld + c;
    *at = apply_col(p, s_mean, s_den, c, *at);
  }
}

// ---------------------------------------------------------------- raw-store process_step
// her_process_step_body's statistics half, call for call (threads 128 .. 128 + G: the goal normaliser, beside the observation columns),
// then every env's transition written to its staging record raw: [obs | dg | a] [next_obs | next_dg] [r | d] [next_ag].
__device__ inline void process_step_raw_body(const gcrl::ProcRawArgs& p, const float* raw, const float* pay) {
  const int n = p.n, D = p.D, G = p.G;
  const float* obs = raw; const float* nobs = obs + (size_t)n * D;
  const float* dg = nobs + (size_t)n * D; const float* ndg = dg + (size_t)n * G;
  if (p.gmean && p.gupdate && threadIdx.x >= 128 && threadIdx.x < 128 + G) {
    const int j = threadIdx.x - 128;
    double m = p.gmean[j], v = p.gvar[j];
    int md = p.gmode;
    gcrl::norm_update_col(m, v, 4 * n, G, *p.gcount, md, [&](int i) { return dg[(size_t)i * G + j]; });   // [dg ; next_dg ; ag ; next_ag] lie in this order
    p.gmean[j] = m; p.gvar[j] = v;
  }
  if (p.mean && p.update) {
    for (int j = threadIdx.x; j < D; j += 256) {
      double m = p.mean[j], v = p.var[j];
      int md = p.mode;
      gcrl::norm_update_col(m, v, 2 * n, D, *p.count, md, [&](int i) { return obs[(size_t)i * D + j]; });
      p.mean[j] = m; p.var[j] = v;
    }
  }
  __syncthreads();
  if (p.mean && p.update && threadIdx.x == 0) *p.count = *p.count + (double)(2 * n);   // every column has read the old count
  if (p.gmean && p.gupdate && threadIdx.x == 128) *p.gcount = *p.gcount + (double)(4 * n);
  const int o_ns = p.SA4, o_r = p.SA4 + p.S4, RW = o_r + 2, W = RW + G;
  for (int e = threadIdx.x; e < n * W; e += 256) {
    const int i = e / W, c = e - i * W;
    const float* pw = pay + (long long)i * kPayW;
    const int t = __float_as_int(pw[0]);
    float v = 0.f;
    if (c < D) v = obs[(size_t)i * D + c];
    else if (c < p.S) v = dg[(size_t)i * G + (c - D)];
    else if (c < p.S + p.A) v = pw[3 + (c - p.S)];
    else if (c >= o_ns && c < o_ns + D) v = nobs[(size_t)i * D + (c - o_ns)];
    else if (c >= o_ns + D && c < o_ns + p.S) v = ndg[(size_t)i * G + (c - o_ns - D)];
    else if (c == o_r) v = pw[1];
    else if (c == o_r + 1) v = pw[2];
    else if (c >= RW) v = pw[3 + p.A + (c - RW)];
    p.stage[((long long)(p.env0 + i) * p.flush_len + t) * p.RG + c] = v;
  }
}
__global__ __launch_bounds__(256) void her_process_step_raw_kernel(gcrl::ProcRawArgs p) { process_step_raw_body(p, p.raw, p.pay); }
struct ProcRawInline { gcrl::ProcRawArgs p; int raw_floats; float data[gcrl::kProcRawInlineFloats]; };
static_assert(sizeof(ProcRawInline) <= 4096, "kernel arguments are limited to 4 KB");
__global__ __launch_bounds__(256) void her_process_step_raw_inline_kernel(ProcRawInline q) { process_step_raw_body(q.p, q.data, q.data + q.raw_floats); }
__global__ __launch_bounds__(256) void her_process_step_raw_pop_kernel(const gcrl::ProcRawArgs* tab, const float* data, int stride, int raw_floats) {
  const gcrl::ProcRawArgs& p = tab[blockIdx.x];
  const float* d = data + (size_t)blockIdx.x * stride;
  process_step_raw_body(p, d, d + raw_floats);
}

bool fill(const gcrl_normalizer* nz_obs, const gcrl_normalizer* nz_dg, int D, int S, NormArgs* p) {
  std::memset(p, 0, sizeof(*p));
  p->D = D; p->S = S;
  gcrl::normalizer_view(nz_obs, &p->mean, &p->var, nullptr, &p->clip, &p->mode);
  gcrl::normalizer_view(nz_dg, &p->gmean, &p->gvar, nullptr, &p->gclip, &p->gmode);
  p->lo = p->mean ? 0 : p->D;
  p->hi = p->gmean ? p->S : p->D;
  return p->lo < p->hi;
}

// n rows of up to three matrices (null ones skipped), each with its own stride, in ONE launch: the quad kernel when every matrix
// allows 16-byte accesses (base aligned, stride a multiple of 4 floats that holds the last quad), the element kernel otherwise
int launch(const gcrl_normalizer* nz_obs, const gcrl_normalizer* nz_dg, int D, int S, int64_t n, float* const* x, const int* ld, int mats,
           hipStream_t st) {
  NormArgs p;
  if (n <= 0 || !fill(nz_obs, nz_dg, D, S, &p)) return GCRL_OK;
  p.n = n;
  float** px[3] = {&p.x0, &p.x1, &p.x2};
  int* pl[3] = {&p.ld0, &p.ld1, &p.ld2};
  unsigned m = 0;
  bool quads = true;
  for (int i = 0; i < mats; ++i) {
    if (!x[i]) continue;
    *px[m] = x[i]; *pl[m] = ld[i]; ++m;
    quads = quads && ld[i] % 4 == 0 && ld[i] >= gcrl::round_up(p.hi, 4) && (uintptr_t)x[i] % 16 == 0;
  }
  if (m == 0) return GCRL_OK;
  const dim3 grid((unsigned)((n + kRows - 1) / kRows), m);
  if (quads) hipLaunchKernelGGL(her_norm_rows_kernel, grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL(her_norm_dense_kernel, grid, dim3(256), 0, st, p);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

}  // namespace

namespace gcrl {

bool her_norm_on(const gcrl_her* h) { return h && h->normalize_mode == GCRL_NORMALIZE_SAMPLE; }

int her_norm_check(const gcrl_her* h, const char* who) {
  if (!her_norm_on(h)) return GCRL_OK;
  const bool need_o = (h->norm_need & 1) != 0, need_g = (h->norm_need & 2) != 0;
  if ((need_o && !h->nz_obs) || (need_g && !h->nz_dg) || (!h->nz_obs && !h->nz_dg))
    return fail(GCRL_ERR_STATE, "%s: normalize: the ring stores raw rows (normalize=\"sample\") and its %s normaliser is not bound: a batch "
                                "cannot be normalised (gcrl_her_set_normalize)", who, (need_o || !need_g) && !h->nz_obs ? "observation" : "goal");
  return GCRL_OK;
}

int her_norm_rows(const gcrl_her* h, int64_t n, float* sa, float* nsa, float* spa, int ldx, hipStream_t st) {
  if (!her_norm_on(h) || n <= 0) return GCRL_OK;
  if (int rc = her_norm_check(h, "gather")) return rc;
  float* const x[3] = {sa, nsa, spa};
  const int ld[3] = {ldx, ldx, ldx};   // (the engine's matrices: 16-byte aligned, stride roundup(S + A, 4) — the quad kernel)
  return launch(h->nz_obs, h->nz_dg, h->norm_D, h->S, n, x, ld, 3, st);
}

int her_norm_dense(const gcrl_her* h, int64_t n, float* out_s, int ld_s, float* out_ns, int ld_ns, hipStream_t st) {
  if (!her_norm_on(h) || n <= 0) return GCRL_OK;
  if (int rc = her_norm_check(h, "sample")) return rc;
  float* const x[2] = {out_s, out_ns};
  const int ld[2] = {ld_s, ld_ns};
  return launch(h->nz_obs, h->nz_dg, h->norm_D, h->S, n, x, ld, 2, st);
}

int her_process_step_raw(const ProcRawArgs& p, const float* data, int raw_floats, int floats, hipStream_t st) {
  if (data) {
    if (floats < 0 || floats > kProcRawInlineFloats || raw_floats < 0 || raw_floats > floats)
      return fail(GCRL_ERR_ARG, "her_process_step_raw: %d inline floats (max %d)", floats, kProcRawInlineFloats);
    ProcRawInline q;
    q.p = p; q.raw_floats = raw_floats;
    std::memcpy(q.data, data, sizeof(float) * (size_t)floats);
    hipLaunchKernelGGL(her_process_step_raw_inline_kernel, dim3(1), dim3(256), 0, st, q);
  } else hipLaunchKernelGGL(her_process_step_raw_kernel, dim3(1), dim3(256), 0, st, p);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

int her_process_step_raw_pop(const ProcRawArgs* tab_dev, const float* data_dev, int stride, int raw_floats, int members, hipStream_t st) {
  hipLaunchKernelGGL(her_process_step_raw_pop_kernel, dim3(members), dim3(256), 0, st, tab_dev, data_dev, stride, raw_floats);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

}  // namespace gcrl

extern "C" {

int gcrl_her_set_normalize(gcrl_her* h, gcrl_normalizer* nz_obs, gcrl_normalizer* nz_dg, int obs_dim) {
  GCRL_CHECK_ARG(h, "gcrl_her_set_normalize: null handle");
  GCRL_CHECK_ARG(obs_dim >= 1 && obs_dim <= 128 && obs_dim + h->G == h->S,
                 "gcrl_her_set_normalize: normalize: obs_dim %d + goal_dim %d != state_dim %d (obs_dim <= 128)", obs_dim, h->G, h->S);
  GCRL_CHECK_ARG(h->S <= kMaxS && h->G <= kMaxG, "gcrl_her_set_normalize: normalize: state_dim %d > %d", h->S, kMaxS);
  GCRL_CHECK_ARG(!nz_obs || gcrl_normalizer_size(nz_obs) == obs_dim,
                 "gcrl_her_set_normalize: normalize: observation normaliser of size %d for obs_dim %d", gcrl_normalizer_size(nz_obs), obs_dim);
  GCRL_CHECK_ARG(!nz_dg || gcrl_normalizer_size(nz_dg) == h->G,
                 "gcrl_her_set_normalize: normalize: goal normaliser of size %d for goal_dim %d", gcrl_normalizer_size(nz_dg), h->G);
  GCRL_CHECK_ARG(!gcrl::per_is_td(h->per) || gcrl::per_is_her_td(h->per), "gcrl_her_set_normalize: normalize: a ring with a TD priority tree (PER) stores what it is given; "
                                           "sample-time normalisation is a HER ring's");
  if (h->normalize_mode != GCRL_NORMALIZE_SAMPLE) {
    bool staged = false;
    for (int v : h->staged) staged = staged || v != 0;
    GCRL_CHECK_ARG(h->rows_pushed == 0 && h->len == 0 && !staged,
                   "gcrl_her_set_normalize: normalize: the ring already holds rows pushed in the other mode (%lld pushed, %lld live%s)",
                   (long long)h->rows_pushed, (long long)h->len, staged ? ", episodes staged" : "");
  } else GCRL_CHECK_ARG(obs_dim == h->norm_D, "gcrl_her_set_normalize: normalize: obs_dim %d, the ring was marked raw with obs_dim %d", obs_dim, h->norm_D);
  h->normalize_mode = GCRL_NORMALIZE_SAMPLE;
  h->nz_obs = nz_obs; h->nz_dg = nz_dg; h->norm_D = obs_dim;
  return GCRL_OK;
}

int gcrl_her_require_normalize(gcrl_her* h, int need_obs, int need_dg) {
  GCRL_CHECK_ARG(h, "gcrl_her_require_normalize: null handle");
  if (h->normalize_mode != GCRL_NORMALIZE_SAMPLE)
    return gcrl::fail(GCRL_ERR_STATE, "gcrl_her_require_normalize: normalize: the ring is not in GCRL_NORMALIZE_SAMPLE (gcrl_her_set_normalize)");
  h->norm_need = (need_obs ? 1 : 0) | (need_dg ? 2 : 0);
  return GCRL_OK;
}

int gcrl_her_normalize_mode(const gcrl_her* h) { return h ? h->normalize_mode : -1; }

int gcrl_normalizer_normalize_states(gcrl_normalizer* nz_obs, gcrl_normalizer* nz_dg, int obs_dim, int state_dim, int64_t n, float* x0, int ld0,
                                     float* x1, int ld1, float* x2, int ld2, void* stream) {
  GCRL_CHECK_ARG(nz_obs || nz_dg, "gcrl_normalizer_normalize_states: no normaliser");
  GCRL_CHECK_ARG(obs_dim >= 1 && obs_dim <= 128 && state_dim > obs_dim && state_dim - obs_dim <= kMaxG,
                 "gcrl_normalizer_normalize_states: obs_dim %d (1..128), state_dim %d (goal_dim 1..%d)", obs_dim, state_dim, kMaxG);
  GCRL_CHECK_ARG(!nz_obs || gcrl_normalizer_size(nz_obs) == obs_dim, "gcrl_normalizer_normalize_states: observation normaliser of size %d for obs_dim %d",
                 gcrl_normalizer_size(nz_obs), obs_dim);
  GCRL_CHECK_ARG(!nz_dg || gcrl_normalizer_size(nz_dg) == state_dim - obs_dim, "gcrl_normalizer_normalize_states: goal normaliser of size %d for goal_dim %d",
                 gcrl_normalizer_size(nz_dg), state_dim - obs_dim);
  GCRL_CHECK_ARG(n >= 0 && (x0 || x1 || x2), "gcrl_normalizer_normalize_states: no rows");
  GCRL_CHECK_ARG((!x0 || ld0 >= state_dim) && (!x1 || ld1 >= state_dim) && (!x2 || ld2 >= state_dim), "gcrl_normalizer_normalize_states: row stride smaller than state_dim %d", state_dim);
  float* const x[3] = {x0, x1, x2};
  const int ld[3] = {ld0, ld1, ld2};
  return launch(nz_obs, nz_dg, obs_dim, state_dim, n, x, ld, 3, stream == GCRL_STREAM_LEGACY ? (hipStream_t) nullptr : (hipStream_t)stream);
}

}  // extern "C"
