// her_prior.hip — prior-data replay: a fixed share of every batch from a second ring (prior_buffer / prior_rows).
//
// Every batch of B rows an agent gathers from its own ring keeps rows [0, B - Bd) as that gather wrote them; rows [B - Bd, B) of batch
// j become batch j of the prior ring's own gather of Bd rows per batch.  Nothing here gathers: the prior ring's existing
// her_gather_update (whatever family its configuration selects, its normalise pass included) writes the rows of a gather part into
// a scratch batch, contiguously, and
//   her_place_rows_kernel   ONE launch per gather part copies scratch row t into row (B - Bd) + t % Bd of batch slot b0 + t / Bd of
//       sa / nsa / spa / r / d.  Row payloads travel as 16-byte quads (ldx is a multiple of 4), r and d as single floats, so B - Bd
//       need not be a multiple of 4.  sa: all ldx columns; nsa: the record's next-state group, zeros behind it ("nsa = [ns | 0..]",
//       which the gathers' partial last wave leaves unwritten in the scratch); spa: the roundup(S, 4) columns its gather writes.
//       Every address comes from the kernel arguments alone, never from data.
// The mapping and the counters of a call are prior_host.h (HIP-free, checked on the host under sanitizers); the rule is restated in
// numpy in tests/her_prior_ref.py, which is its definition.
//
// A translation unit of its own: every other unit's kernels keep their code, byte for byte.  The kernel has an exact grid, no LDS,
// no waits between workgroups, no atomics and no per-thread scratch.
#include "her_prior.h"
#include "per_tree.h"

namespace {

struct PlaceArgs {
  const float *psa, *pnsa, *pspa, *pr, *pd;   // the scratch rows of this launch, contiguous (pspa null: no spa)
  float *sa, *nsa, *spa, *r, *d;              // the launch's first batch slot
  gcrl::PriorPlace pl;
  int ldq, s4q, spq;                          // quads of a row; of its state group roundup(S, 4); of spa's part (0 or s4q)
  long long rows;                             // scratch rows of this launch: a multiple of pl.Bd
};

// Thread t: unit u = t % U of scratch row t / U, U = 2 ldq + spq + 1 — the ldq quads of sa, the ldq quads of nsa, the spq quads of
// spa, then r and d.  Bounds: row < rows, so the scratch reads end below rows * ldx (rows) floats; the destination row lies in
// slot row / Bd < rows / Bd at row index < B, inside the slots the host checked against the batch matrices.
__global__ __launch_bounds__(256) void her_place_rows_kernel(PlaceArgs p) {
  const int U = 2 * p.ldq + p.spq + 1;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= p.rows * U) return;
  const long long row = t / U;
  const int u = (int)(t - row * U);
  const long long src = row * p.pl.ldx;
  if (u == U - 1) {
    const long long o = gcrl::prior_rd_offset(p.pl, row);
    p.r[o] = p.pr[row];
    p.d[o] = p.pd[row];
    return;
  }
  const long long dst = gcrl::prior_x_offset(p.pl, row);
  if (u < p.ldq) {
    *reinterpret_cast<float4*>(p.sa + dst + 4 * u) = *reinterpret_cast<const float4*>(p.psa + src + 4 * u);
  } else if (u < 2 * p.ldq) {
    const int q = u - p.ldq;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q < p.s4q) v = *reinterpret_cast<const float4*>(p.pnsa + src + 4 * q);
    *reinterpret_cast<float4*>(p.nsa + dst + 4 * q) = v;
  } else {
    const int q = u - 2 * p.ldq;
    *reinterpret_cast<float4*>(p.spa + dst + 4 * q) = *reinterpret_cast<const float4*>(p.pspa + src + 4 * q);
  }
}

}  // namespace

namespace gcrl {

int her_prior_check_ring(const gcrl_her* prior, int S, int A, int B, int Bd, const char* who) {
  if (!prior) return fail(GCRL_ERR_ARG, "%s: prior_buffer: null ring", who);
  if (!prior_rows_ok(B, Bd)) return fail(GCRL_ERR_ARG, "%s: prior_rows: %d rows of a batch of %d (1..%d)", who, Bd, B, B - 1);
  if (prior->cfg.rng_mode != GCRL_RNG_DEVICE)
    return fail(GCRL_ERR_ARG, "%s: prior_buffer: the prior ring's gather computes its own row indices and needs rng=\"device\"", who);
  if (prior->per) return fail(GCRL_ERR_ARG, "%s: prior_buffer: the prior ring carries a priority tree; it is drawn uniformly", who);
  if (prior->S != S || prior->A != A)
    return fail(GCRL_ERR_ARG, "%s: prior_buffer: the prior ring's dims (S=%d,A=%d) differ from (S=%d,A=%d)", who, prior->S, prior->A, S, A);
  return GCRL_OK;
}

int her_prior_check_call(const gcrl_her* main_ring, const gcrl_her* prior, int Bd, const char* who) {
  if (prior == main_ring) return fail(GCRL_ERR_STATE, "%s: prior_buffer: the prior ring is the ring it is mixed into", who);
  if (prior->S != main_ring->S || prior->A != main_ring->A || prior->G != main_ring->G)
    return fail(GCRL_ERR_STATE, "%s: prior_buffer: the prior ring's dims (S=%d,A=%d,G=%d) differ from the main ring's (S=%d,A=%d,G=%d)", who,
                prior->S, prior->A, prior->G, main_ring->S, main_ring->A, main_ring->G);
  if (per_is_her_td(main_ring->per))
    return fail(GCRL_ERR_STATE, "%s: prioritise: a main ring with a TD-error tree weighs and re-prioritises every row it draws; prior rows have no leaf", who);
  if (per_is_td(main_ring->per))
    return fail(GCRL_ERR_STATE, "%s: prior_buffer: a main ring with a TD priority tree weighs and re-prioritises every row it draws; prior rows have no leaf", who);
  if (her_norm_on(prior) != her_norm_on(main_ring))
    return fail(GCRL_ERR_STATE, "%s: prior_buffer: the prior ring's normalize mode differs from the main ring's (raw and normalised rows would share a batch)", who);
  if (prior->cfg.rng_mode != GCRL_RNG_DEVICE || prior->per)
    return fail(GCRL_ERR_STATE, "%s: prior_buffer: the prior ring needs rng=\"device\" and no priority tree", who);
  if (prior->len < Bd)
    return fail(GCRL_ERR_NOT_ENOUGH, "[ERROR] Not enough in buffer to sample (prior_buffer holds %lld rows, prior_rows = %d)", (long long)prior->len, Bd);
  char name[96];
  std::snprintf(name, sizeof(name), "%s: prior_buffer", who);
  return her_norm_check(prior, name);
}

PriorSnap her_prior_take(gcrl_her* prior, int n, int Bd) {
  PriorSnap s;
  s.draw0 = prior->draws_done;
  s.ctr0 = prior->relabel_ctr;
  s.len = (uint32_t)prior->len;
  s.Bd = Bd;
  prior->draws_done += prior_draws_of(n);
  if (prior->relabel_mode == GCRL_RELABEL_SAMPLE) prior->relabel_ctr += prior_rows_of(n, Bd);
  return s;
}

int her_prior_gather_place(gcrl_her* prior, const PriorSnap& snap, int b0, int nb, double gamma, const PriorScratch& sc, float* sa,
                           float* nsa, float* spa, float* r, float* d, const PriorPlace& pl, hipStream_t st) {
  if (nb <= 0) return GCRL_OK;
  if (b0 < 0 || !prior_rows_ok(pl.B, pl.Bd) || snap.Bd != pl.Bd || pl.ldx != prior->SA4 || pl.ldx % 4 != 0 || (spa && !sc.spa))
    return fail(GCRL_ERR_ARG, "her_prior_gather_place: prior_rows: bad placement (b0=%d, B=%d, Bd=%d, ldx=%d)", b0, pl.B, pl.Bd, pl.ldx);
  const PriorPart part = prior_part(snap, b0, nb);
  const long long off = (long long)b0 * pl.Bd;
  float* psa = sc.sa + off * pl.ldx;
  float* pnsa = sc.nsa + off * pl.ldx;
  float* pspa = spa ? sc.spa + off * pl.ldx : nullptr;
  prior->last_gen = IdxGen{prior->cfg.seed, part.draw, snap.len, pl.Bd, feistel_half_bits(snap.len)};
  if (int rc = her_gather_update(prior, nullptr, part.rows, psa, pnsa, pspa, pl.ldx, sc.r + off, sc.d + off, st, nullptr, nullptr, 0, &part.ctr, &gamma))
    return rc;
  PlaceArgs p{psa, pnsa, pspa, sc.r + off, sc.d + off,
              sa + b0 * pl.slot_x, nsa + b0 * pl.slot_x, spa ? spa + b0 * pl.slot_x : nullptr, r + b0 * pl.slot_rd, d + b0 * pl.slot_rd,
              pl, pl.ldx / 4, prior->S4 / 4, spa ? prior->S4 / 4 : 0, part.rows};
  const long long total = part.rows * (2 * p.ldq + p.spq + 1);
  hipLaunchKernelGGL(her_place_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

}  // namespace gcrl

extern "C" int gcrl_her_gather_update_mixed(gcrl_her* main_ring, gcrl_her* prior, int B, int Bd, int M, float* sa, float* nsa, float* spa, int ldx,
                                            float* r, float* d, void* stream) {
  using namespace gcrl;
  const char* who = "gcrl_her_gather_update_mixed";
  GCRL_CHECK_ARG(main_ring && sa && nsa && r && d, "gcrl_her_gather_update_mixed: null argument");
  GCRL_CHECK_ARG(B >= 1 && M >= 1, "gcrl_her_gather_update_mixed: B and M must be >= 1");
  if (int rc = her_prior_check_ring(prior, main_ring->S, main_ring->A, B, Bd, who)) return rc;
  GCRL_CHECK_ARG(ldx == main_ring->SA4, "gcrl_her_gather_update_mixed: batch row stride %d != roundup(S+A,4) = %d", ldx, main_ring->SA4);
  if (int rc = her_prior_check_call(main_ring, prior, Bd, who)) return rc;
  if (main_ring->len < B) return fail(GCRL_ERR_NOT_ENOUGH, "[ERROR] Not enough in buffer to sample");
  hipStream_t st = main_ring->pick(stream);
  PriorScratch sc;
  const size_t rows = (size_t)M * Bd, xf = rows * (size_t)ldx;
  float* block = nullptr;
  GCRL_HIP(hipMalloc((void**)&block, ((spa ? 3 : 2) * xf + 2 * rows) * sizeof(float)));
  sc.sa = block; sc.nsa = block + xf; sc.spa = spa ? block + 2 * xf : nullptr;
  sc.r = block + (spa ? 3 : 2) * xf; sc.d = sc.r + rows;
  int rc = gcrl_her_gather_update(main_ring, B, M, nullptr, sa, nsa, spa, ldx, r, d, nullptr, nullptr, 0, stream);
  if (!rc) {
    const PriorSnap snap = her_prior_take(prior, M, Bd);
    const PriorPlace pl{B, Bd, ldx, (long long)B * ldx, (long long)B};
    rc = her_prior_gather_place(prior, snap, 0, M, prior->nstep_gamma, sc, sa, nsa, spa, r, d, pl, st);
  }
  const hipError_t e = hipStreamSynchronize(st);
  (void)hipFree(block);
  if (!rc && e != hipSuccess) return fail(GCRL_ERR_HIP, "gcrl_her_gather_update_mixed: %s", hipGetErrorString(e));
  return rc;
}
