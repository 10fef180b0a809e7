// her_prior.h — prior-data replay (her_prior.hip): what the update engine needs of it.
#pragma once
#include "her_ring.h"
#include "prior_host.h"

namespace gcrl {

// what gcrl_agent_set_prior / gcrl_her_gather_update_mixed ask of a prior ring, each refusal naming prior_buffer or prior_rows
int her_prior_check_ring(const gcrl_her* prior, int S, int A, int B, int Bd, const char* who);
// ... and what a call asks of it against the ring it is mixed into, before anything is consumed
int her_prior_check_call(const gcrl_her* main_ring, const gcrl_her* prior, int Bd, const char* who);

// the prior ring's counters as of now (a PriorSnap), advanced by a call of n batches of Bd rows
PriorSnap her_prior_take(gcrl_her* prior, int n, int Bd);

// the scratch batch of an agent: [Mmax * Bd] rows of sa, nsa, spa (null where the agent has none), r, d
struct PriorScratch {
  float *sa = nullptr, *nsa = nullptr, *spa = nullptr, *r = nullptr, *d = nullptr;
};

// One gather part: batches [b0, b0 + nb) of the call whose counters `snap` holds.  The prior ring's own her_gather_update writes
// their nb * Bd rows into the scratch at row b0 * Bd, then ONE her_place_rows_kernel launch copies them into rows [B - Bd, B) of
// batch slots b0 .. b0 + nb - 1 of sa / nsa / spa / r / d (the bases of slot 0; spa may be null).  At most two launches (three when
// the prior ring is normalize = "sample": its in-place pass over the scratch).
int her_prior_gather_place(gcrl_her* prior, const PriorSnap& snap, int b0, int nb, double gamma, const PriorScratch& sc, float* sa,
                           float* nsa, float* spa, float* r, float* d, const PriorPlace& pl, hipStream_t st);

}  // namespace gcrl
