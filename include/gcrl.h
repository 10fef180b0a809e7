/*
 * gcrl.h — C ABI of libgcrl_hip.so: MI355X-native HER replay + actor-critic update engine.
 *
 * The reference (CodeKnight314/Goal-Conditioned-RL-Framework) has NO native/FFI layer: its
 * boundary is the duck-typed Python surface that src/env.py uses on `agent` and `agent.buffer`
 * (SURVEY.md §8b).  Each entry point below therefore cites the reference *Python* method it
 * replaces; the Python classes in goal-conditioned-rl-framework_amd/src/ (same names and
 * signatures as the reference's) are thin ctypes callers of these functions.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / C++ types.  `*_dev` = device (HBM) pointer,
 *     `*_host` = host pointer.  `stream` is a hipStream_t passed as void*: NULL = the
 *     handle's own (non-blocking) stream, GCRL_STREAM_LEGACY = HIP's legacy default stream
 *     (what torch.cuda.current_stream().cuda_stream == 0 means).
 *   - every function returning int returns GCRL_OK (0) or a negative gcrl_status; nothing
 *     throws across the boundary.  gcrl_last_error() gives the message (thread-local).
 *   - one calling thread per handle (the reference's trainer is single-threaded,
 *     src/env.py:334-406); all device work of a handle is stream-ordered.
 *   - there is NO CPU fallback: every device entry point fails with GCRL_ERR_HIP when no
 *     gfx950 device is usable.  Host-only entry points (gcrl_mt_*, gcrl_cosine_lr_*) work
 *     without a GPU.
 */
#ifndef GCRL_H
#define GCRL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCRL_ABI_VERSION 1
#define GCRL_STREAM_LEGACY ((void*)1)

typedef enum gcrl_status {
  GCRL_OK = 0,
  GCRL_ERR_ARG = -1,        /* bad argument / unsupported shape */
  GCRL_ERR_HIP = -2,        /* HIP runtime error (message has hipGetErrorString) */
  GCRL_ERR_NOT_ENOUGH = -3, /* sample(B) with len < B  (reference: assert, src/buffer.py:122) */
  GCRL_ERR_STATE = -4       /* call made in the wrong state */
} gcrl_status;

const char* gcrl_last_error(void);
int gcrl_abi_version(void);
/* number of usable HIP devices (0 when none); never fails */
int gcrl_device_count(void);

/* ------------------------------------------------------------------------------------------
 * CPython-exact Mersenne Twister.  Replaces the stdlib `random` calls the reference makes on
 * the hot path: random.randint (src/buffer.py:153) and random.sample (src/buffer.py:124);
 * random.random (src/agent.py:1348) shares the same stream.  Algorithm: CPython 3.10
 * Lib/random.py (_randbelow_with_getrandbits, sample, randrange) + Modules/_randommodule.c
 * (init_by_array, genrand_uint32, genrand_res53).  Host-only.
 * ---------------------------------------------------------------------------------------- */
typedef struct gcrl_mt gcrl_mt;

gcrl_mt* gcrl_mt_create(void);
void gcrl_mt_destroy(gcrl_mt* mt);
/* random.seed(n) for a non-negative int n < 2**64 */
int gcrl_mt_seed(gcrl_mt* mt, uint64_t seed);
/* state[0..623] = MT words, state[624] = index; same layout as random.getstate()[1] */
int gcrl_mt_get_state(const gcrl_mt* mt, uint32_t* state625);
int gcrl_mt_set_state(gcrl_mt* mt, const uint32_t* state625);
uint32_t gcrl_mt_getrandbits(gcrl_mt* mt, int k /* 1..32 */);
uint32_t gcrl_mt_randbelow(gcrl_mt* mt, uint32_t n /* >= 1 */);
int64_t gcrl_mt_randint(gcrl_mt* mt, int64_t a, int64_t b); /* a + randbelow(b-a+1) */
double gcrl_mt_random(gcrl_mt* mt);
/* index stream of random.sample(population_of_len_n, k): out[i] = index chosen i-th.
 * Both the pool path (n <= setsize(k)) and the set path are reproduced. */
int gcrl_mt_sample_indices(gcrl_mt* mt, uint32_t n, uint32_t k, uint32_t* out_host);
/* draw order of HERBuffer.apply_her (src/buffer.py:146-153): for i in 0..T-2, k_future times
 * randint(i+1, T-1); nothing for the last step.  out has k_future*(T-1) entries. */
int gcrl_mt_future_indices(gcrl_mt* mt, int T, int k_future, uint8_t* out_host);

/* ------------------------------------------------------------------------------------------
 * torch.optim.lr_scheduler.CosineAnnealingLR (recursive/"chainable" form) as the reference
 * configures it (src/agent.py:1203-1212 etc.).  Host-only, double precision like torch.
 * lr_after_k_steps: lr used by the optimiser step number k+1 (k scheduler.step() calls done).
 * ---------------------------------------------------------------------------------------- */
double gcrl_cosine_lr_next(double lr_now, double base_lr, double eta_min, int64_t t_max,
                           int64_t last_epoch_after_step);

/* ------------------------------------------------------------------------------------------
 * HER replay ring in HBM.  Replaces class HERBuffer (src/buffer.py:92-179).
 * Layout (fp32): one 64-byte-aligned packed record per transition,
 * [s(S)|a(A)|pad4][ns(S)|pad4][r|d|pad] (every field group 16-byte aligned),
 * records contiguous in arrival order (DESIGN.md "HBM layout" explains why not five field
 * arrays: a random row gather would touch ~3x the 128-B lines).  sample() returns the five
 * dense field matrices of the reference.  The stored dg/ag columns of the reference's tuples
 * are never read by sample() (src/buffer.py:125) and are not materialised.
 * ---------------------------------------------------------------------------------------- */
typedef struct gcrl_her gcrl_her;

/* GCRL_REWARD_HOST: any other callable.  The reference calls whatever was injected (src/env.py:105) once per relabelled row
 * (src/buffer.py:166); with this kind the flush does the same through gcrl_her_set_reward_callback: the picks and the goal
 * swap stay on the device, the rewards of a flush launch's relabel slots are computed by the callback on the host (from a
 * host mirror of the staged achieved goals) and uploaded with the launch. */
enum { GCRL_REWARD_SPARSE = 0, GCRL_REWARD_DENSE = 1, GCRL_REWARD_HOST = 2 };
enum { GCRL_RNG_CPYTHON_MT = 0, GCRL_RNG_DEVICE = 1 };

typedef struct gcrl_her_config {
  int32_t state_dim;   /* S: obs + time feature + goal (goal = LAST goal_dim entries) */
  int32_t action_dim;  /* A */
  int32_t goal_dim;    /* G */
  int64_t capacity;    /* max_mem_len (deque maxlen, src/buffer.py:101) */
  int32_t nenvs;       /* per-env staging areas (src/buffer.py:102) */
  int32_t k_future;    /* relabels per step (src/buffer.py:151); 1..64 here (gcrl_her_create refuses more: the flush kernel gives a
                        * 16-lane group per stored row and keeps a step's picks in one wave) — the reference has no such limit */
  int32_t flush_len;   /* 50: literal in src/buffer.py:117 (max_eps_len is ignored there) */
  int32_t reward_kind; /* GCRL_REWARD_*: stands in for the injected compute_reward
                          (src/env.py:105, src/buffer.py:166): sparse = -(||ag-g||2 > thr) */
  float reward_threshold; /* 0.05 for all Panda tasks */
  int32_t device;
  int32_t rng_mode;    /* GCRL_RNG_* */
  uint64_t seed;       /* used when the handle owns its RNG */
} gcrl_her_config;

/* rng: shared CPython-exact generator (may be NULL: the handle creates one seeded with
 * cfg->seed).  The ring never frees a shared rng. */
gcrl_her* gcrl_her_create(const gcrl_her_config* cfg, gcrl_mt* rng);
/* Relabelling mode of a ring.  GCRL_RELABEL_PUSH (what gcrl_her_create makes): the reference's form — a flush stores every step's
 * original row and its k_future relabelled copies, `capacity` counts copies.  GCRL_RELABEL_SAMPLE: a flush stores an episode's T
 * original rows once (no future pick is drawn: the CPython-MT stream is not consumed by a flush), each record with a tail
 * [achieved goal | steps remaining in its episode]; `capacity` counts real transitions.  A row is relabelled when it is gathered:
 * with probability k_future / (k_future + 1), against a uniformly chosen later row of its episode, by a counter hash of the number
 * of rows gathered from the ring so far (gcrl_her_get_relabel_counter) — also when the indices come from the CPython-MT stream.
 * Refused: reward_kind GCRL_REWARD_HOST (the relabel rewards are computed in the gather kernel), gcrl_per_attach on such a ring,
 * gcrl_her_load_state of a blob saved in the other mode. */
enum { GCRL_RELABEL_PUSH = 0, GCRL_RELABEL_SAMPLE = 1 };
gcrl_her* gcrl_her_create_relabel(const gcrl_her_config* cfg, gcrl_mt* rng, int mode);
int gcrl_her_relabel_mode(const gcrl_her* h);
/* rows ever gathered from a GCRL_RELABEL_SAMPLE ring: the counter of its relabel stream (saved and loaded with the ring's state) */
uint64_t gcrl_her_get_relabel_counter(const gcrl_her* h);
int gcrl_her_set_relabel_counter(gcrl_her* h, uint64_t counter);
/* n-step returns on a GCRL_RELABEL_SAMPLE ring: n_step = N in 1..8 (1, the default: one-step rows).  With
 * N > 1 a gathered row p becomes a window of m = min(N, remaining + 1) rows of its episode: s, a of row p, ns of row p + m - 1,
 * r <- sum_j gamma^j r_j (each r_j recomputed against the new goal when the row is relabelled, otherwise as stored) and
 * d <- 1 - gamma^(m-1) (1 - d_last), so that the engine's r + gamma (1 - d) q' is the n-step target.  The relabel decision and the
 * counter are consumed as for N = 1.  `gamma` is the discount of the ring's own gathers (gcrl_her_sample, gcrl_her_sample_dev,
 * gcrl_her_gather_update), applied as a float; an agent's update calls discount by the agent's gamma as of the call.
 * Configuration, not state: gcrl_her_save_state / gcrl_her_load_state do not carry it.  Refused, naming n_step: a value outside
 * 1..8 (GCRL_ERR_ARG), N > 1 on a GCRL_RELABEL_PUSH ring (GCRL_ERR_STATE).  gcrl_her_get_nstep returns N (gamma through *gamma,
 * which may be NULL), -1 for a null handle. */
int gcrl_her_set_nstep(gcrl_her* h, int n_step, double gamma);
int gcrl_her_get_nstep(const gcrl_her* h, double* gamma);
/* Goal selection of a GCRL_RELABEL_SAMPLE ring (csrc/her_relabel.hip; tests/her_strategy_ref.py is the definition):
 * WHICH row of its episode a relabelled row takes its goal from.  GCRL_GOAL_FUTURE (what gcrl_her_create_relabel makes): a uniformly
 * chosen later row.  GCRL_GOAL_FINAL: the episode's last row (an episode's last row itself is never relabelled).  GCRL_GOAL_EPISODE:
 * a uniformly chosen OTHER live row of the episode, earlier ones included; its records carry a second tail word,
 * [achieved goal | remaining | elapsed], so the record width differs and the strategy is fixed at creation.  The relabel decision
 * (share k_future / (k_future + 1)), the counter and n-step windows are those of GCRL_GOAL_FUTURE for every strategy.
 * Refused with GCRL_ERR_ARG, naming goal_strategy: an unknown strategy; FINAL or EPISODE on a GCRL_RELABEL_PUSH ring.  A FUTURE ring
 * writes the state blobs of before; another strategy's blob carries the strategy, and gcrl_her_load_state across differing
 * strategies is refused by that name, as is gcrl_pop_clone between such rings. */
enum { GCRL_GOAL_FUTURE = 0, GCRL_GOAL_FINAL = 1, GCRL_GOAL_EPISODE = 2 };
gcrl_her* gcrl_her_create_goal(const gcrl_her_config* cfg, gcrl_mt* rng, int mode, int strategy);
int gcrl_her_goal_strategy(const gcrl_her* h);   /* -1 for a null handle */
/* Sample-time normalisation (csrc/her_norm.hip; tests/her_normalize_ref.py is the definition).  A ring is created
 * in GCRL_NORMALIZE_PUSH: its records hold whatever the caller pushed, which for the trainer is rows normalised with the statistics
 * of the moment of the push.  gcrl_her_set_normalize marks it GCRL_NORMALIZE_SAMPLE ("raw") and binds the two device normalisers —
 * borrowed, never freed by the ring; either may be NULL (those columns stay raw); a later call re-binds.  On a raw ring
 *   - gcrl_her_process_step_g / gcrl_pop_process_step update the statistics as before and stage the rows and achieved goals RAW;
 *   - every reward a gather recomputes (relabelled rows, n-step windows) and the energy tree read raw achieved goals;
 *   - one in-place launch behind every gather (gcrl_her_sample, gcrl_her_sample_dev, gcrl_her_gather_update, the update engine's
 *     and the populations' gathers) normalises columns [0, obs_dim) of s and ns with nz_obs and [obs_dim, state_dim) with nz_dg:
 *     bit for bit gcrl_normalizer_normalize of those columns with the statistics as they stand in stream order at that launch.
 *     Actions, rewards, done flags and padding columns are not touched.
 * Refused with GCRL_ERR_ARG, naming normalize: a normaliser of another size than its columns; obs_dim + goal_dim != state_dim or
 * obs_dim > 128; a ring that already holds or stages rows pushed in the other mode; a ring with a TD priority tree or rows appended
 * one by one (gcrl_her_append: the REPLAY and PER buffers), and gcrl_her_append on a raw ring likewise.
 * gcrl_her_require_normalize says which normalisers a gather must find bound (bit 0: nz_obs, bit 1: nz_dg); a raw ring with neither
 * bound, or without a required one, refuses to gather with GCRL_ERR_STATE naming normalize before a ticket or a counter is
 * consumed.  Also refused by that name: an update call of an agent under a gradient exchange from a raw ring; gcrl_pop_clone
 * between rings of differing modes; gcrl_her_load_state of a blob saved in the other mode (a raw ring's blob carries the flag 0x100 in its version word). */
enum { GCRL_NORMALIZE_PUSH = 0, GCRL_NORMALIZE_SAMPLE = 1 };
struct gcrl_normalizer;   /* (the device RunningNormalizer, declared below) */
int gcrl_her_set_normalize(gcrl_her* h, struct gcrl_normalizer* nz_obs, struct gcrl_normalizer* nz_dg, int obs_dim);
int gcrl_her_require_normalize(gcrl_her* h, int need_obs, int need_dg);
int gcrl_her_normalize_mode(const gcrl_her* h);   /* -1 for a null handle */
/* The pass on its own, for a batch the caller formed (an injected batch of raw states): IN PLACE, columns [0, obs_dim) of every row of
 * the device matrices x0 / x1 / x2 (n rows each, row strides ld0 / ld1 / ld2 floats; NULL matrices are skipped) are normalised with
 * nz_obs and columns [obs_dim, state_dim) with nz_dg (a NULL normaliser leaves its columns as they are); every other column keeps its
 * bits.  One launch: 16-byte accesses when every matrix is 16-byte aligned with a stride that is a multiple of 4 floats and holds
 * roundup(state_dim, 4) columns, element accesses otherwise.  Bit for bit gcrl_normalizer_normalize of those columns. */
int gcrl_normalizer_normalize_states(struct gcrl_normalizer* nz_obs, struct gcrl_normalizer* nz_dg, int obs_dim, int state_dim, int64_t n,
                                     float* x0, int ld0, float* x1, int ld1, float* x2, int ld2, void* stream);
void gcrl_her_destroy(gcrl_her* h);
/* compute_reward for GCRL_REWARD_HOST rings: out[i] = compute_reward(achieved[i], goal[i], {}) for n pairs of goal_dim floats
 * (row-major), in the reference's call order (src/buffer.py:151-166: step-major, relabel-minor).  Returns 0, or non-zero to
 * abort the flush (the push call then fails with GCRL_ERR_STATE).  Called on the pushing thread, inside the push call. */
typedef int (*gcrl_reward_fn)(const float* achieved, const float* goal, int n, int goal_dim, float* out, void* user);
int gcrl_her_set_reward_callback(gcrl_her* h, gcrl_reward_fn fn, void* user);
int64_t gcrl_her_len(const gcrl_her* h);       /* HERBuffer.__len__  src/buffer.py:137 */
int64_t gcrl_her_head(const gcrl_her* h);      /* physical row of logical index 0 */
int32_t gcrl_her_staged(const gcrl_her* h, int env);
void* gcrl_her_stream(const gcrl_her* h);

/* HERBuffer.push (src/buffer.py:110-119).  state/next_state: S floats, either device
 * pointers (the reference passes device tensors, src/env.py:217-219) or host pointers
 * (flag *_on_device).  action (A), desired_goal/achieved_goal (G): host floats.
 * Stages the transition; when `done` or the env has flush_len staged transitions, runs the
 * HER relabel+flush kernel (apply_her) and clears the staging area.
 * Returns the number of ring rows appended (0 = staged only) or a negative status. */
int64_t gcrl_her_push(gcrl_her* h, int env, const float* state, int state_on_device,
                      const float* action_host, const float* next_state,
                      int next_state_on_device, float reward, int done,
                      const float* desired_goal_host, const float* achieved_goal_host,
                      void* stream);

/* ReplayBuffer.push / PERBuffer.push (src/buffer.py:13-14, :46-48): ONE row appended at once (no staging, no relabel,
 * visible to the next sample), deque(maxlen) eviction.  state / next_state: S floats on the device or the host. */
int64_t gcrl_her_append(gcrl_her* h, const float* state, int state_on_device, const float* action_host, float reward,
                        const float* next_state, int next_state_on_device, int done, void* stream);

/* One step of a vector env (the loop of src/env.py:192-201 as ONE call): transition i belongs to
 * env env0+i.  states / next_states: device matrices [n][ld] (what _process_step builds,
 * src/env.py:189-190); actions [n][A], rewards [n], dones [n] (0/1 bytes), achieved goals [n][G]:
 * host.  One payload upload + one staging launch; all envs that finish on this step are relabelled
 * and flushed together (a segment scan over their row counts places each episode), in env order
 * with the RNG draws in env order — identical rows and RNG state to n gcrl_her_push calls.
 * Returns the ring rows appended. */
int64_t gcrl_her_push_batch(gcrl_her* h, int env0, int n, const float* states_dev, int ld_s,
                            const float* actions_host, const float* next_states_dev, int ld_ns,
                            const float* rewards_host, const uint8_t* dones_host,
                            const float* achieved_goals_host, void* stream);

/* Whole-episode variant (one H2D copy + one flush launch): T transitions of env `env` given as
 * host arrays s[T][S], a[T][A], ns[T][S], r[T], d[T] (0/1), ag[T][G].  Equivalent to T calls
 * of gcrl_her_push whose last one triggers the flush; any partially staged episode of that env
 * must be empty.  future_idx (k_future*(T-1) entries, draw order of src/buffer.py:146-153) may
 * be NULL: then drawn from the handle's RNG. */
int64_t gcrl_her_push_episode(gcrl_her* h, int env, int T, const float* s_host,
                              const float* a_host, const float* ns_host, const float* r_host,
                              const float* d_host, const float* ag_host,
                              const uint8_t* future_idx_host, void* stream);

/* HERBuffer.sample (src/buffer.py:121-135), M batches per launch.  Logical indices
 * (0 = oldest row) are drawn by random.sample semantics from the handle's RNG, or taken from
 * idx_host (M*B entries) when non-NULL.  Outputs are device pointers; row strides ld_* in
 * floats (ld_s >= S etc.; rewards/dones are [M*B] contiguous = the reference's [B,1]).
 * drawn_idx_host (optional, M*B) receives the indices used. */
int gcrl_her_sample(gcrl_her* h, int B, int M, const uint32_t* idx_host,
                    float* out_s_dev, int ld_s, float* out_a_dev, int ld_a, float* out_r_dev,
                    float* out_ns_dev, int ld_ns, float* out_d_dev,
                    uint32_t* drawn_idx_host, void* stream);

/* Measurement: when enabled, every gather launch of this ring (gcrl_her_sample and the update
 * engine's batch gather) is bracketed by two hipEvents on the stream it is launched on.
 * gcrl_her_profile_read waits for the pending events and returns, since enabling, for the LARGEST launch size seen (a
 * trainer cycle's main gather; the one-batch head launch that lets step 0 start early is not counted), the number
 * of gather launches, their summed hipEvent time (ms, includes the event/dispatch overhead of a
 * bracketed launch: ~3-4 us more than rocprofv3's kernel duration) and the rows they gathered.  device_clock_ms_out is
 * always 0 now: rounds 1-2 stamped the device wall clock in the first / last blocks, which excludes dispatch and drain and
 * read ~half of the profiler's duration — bench.py takes the kernel's duration from rocprofv3 itself instead. */
int gcrl_her_profile_enable(gcrl_her* h, int on);
int gcrl_her_profile_read(gcrl_her* h, int64_t* launches_out, double* total_ms_out,
                          int64_t* rows_out, double* device_clock_ms_out);

/* Full resume state of the ring (extension of SURVEY.md §8f-2: the reference checkpoints weights + normalisers only,
 * src/env.py:430-440): every stored row in logical order, the per-env staged partial episodes, the counters of the
 * device-RNG mode.  The CPython-MT stream is saved with gcrl_mt_get_state.  Load into a ring of the same shape (any
 * capacity >= the saved row count); logical indices — what sample() draws — are preserved. */
int64_t gcrl_her_state_size(const gcrl_her* h);
int gcrl_her_save_state(gcrl_her* h, void* dst_host, int64_t nbytes);
int gcrl_her_load_state(gcrl_her* h, const void* src_host, int64_t nbytes);

/* Test/debug: copy `n` ring rows starting at logical index `first` to host arrays
 * (any may be NULL).  Synchronises the handle's stream. */
int gcrl_her_read_rows(gcrl_her* h, int64_t first, int64_t n, float* s_host, float* a_host,
                       float* ns_host, float* r_host, float* d_host);
/* The update engine's batch gather on its own (tests, tools): M batches of B rows drawn as gcrl_her_sample draws them (idx_host,
 * the CPython-MT stream or the device RNG) into the engine's GEMM-ready device matrices of row stride ldx = roundup(S + A, 4):
 * sa = [s | a], nsa = [ns | 0 ..], spa (may be NULL) = [s | ..] in its roundup(S, 4) leading columns, r[B * M], d[B * M].
 * side_bytes > 0 (a multiple of 16): the launch also copies side_bytes from side_src to side_dst (both readable / writable by the
 * device) — the engine's call-start form.  A GCRL_RELABEL_SAMPLE ring relabels the rows and advances its counter by B * M. */
int gcrl_her_gather_update(gcrl_her* h, int B, int M, const uint32_t* idx_host, float* sa_dev, float* nsa_dev, float* spa_dev, int ldx,
                           float* r_dev, float* d_dev, const void* side_src, void* side_dst, int64_t side_bytes, void* stream);
/* Test/state: the tails of `n` rows of a GCRL_RELABEL_SAMPLE ring from logical index `first`: ag_host[n][goal_dim],
 * remaining_host[n] (either may be NULL).  Synchronises the device. */
int gcrl_her_read_tails(gcrl_her* h, int64_t first, int64_t n, float* ag_host, float* remaining_host);
/* The same for the `elapsed` word of a GCRL_GOAL_EPISODE ring: elapsed_host[n], the number of rows of its episode that precede each
 * row.  GCRL_ERR_STATE, naming goal_strategy, on a ring whose records have no such word. */
int gcrl_her_read_elapsed(gcrl_her* h, int64_t first, int64_t n, float* elapsed_host);

/* ------------------------------------------------------------------------------------------
 * Update engine.  Replaces DDPG / TD3Agent / SACAgent / TQCAgent .update() and what it calls
 * (src/agent.py:1378-1404, :281-317, :659-699, :1062-1100) plus the networks of src/model.py.
 * ---------------------------------------------------------------------------------------- */
typedef struct gcrl_agent gcrl_agent;

enum { GCRL_AGENT_DDPG = 0, GCRL_AGENT_TD3 = 1, GCRL_AGENT_SAC = 2, GCRL_AGENT_TQC = 3 };

typedef struct gcrl_agent_config {
  int32_t kind;           /* GCRL_AGENT_* */
  int32_t obs_dim;        /* S = obs + goal, the `obs_dim` ctor argument (src/env.py:120-127) */
  int32_t ac_dim;         /* A */
  int32_t hidden_dim;     /* BaseAgentConfig.hidden_dim (src/utils.py:11) */
  int32_t layer_count;    /* BaseAgentConfig.layer_count */
  int32_t batch_size;
  int32_t num_critics;    /* TQC: 5 (src/agent.py:789); DDPG 1; TD3/SAC 2 */
  int32_t top_drop;       /* TQC: 2 (src/agent.py:790) */
  int32_t ac_update_freq;
  int32_t gradient_step;  /* ctor argument; SAC Polyak cadence (src/agent.py:681) */
  int32_t polyak_every;   /* DDPG: literal 40 (src/agent.py:1397) */
  /* hyper-parameters are Python floats (doubles) in the reference's pydantic config */
  double gamma, tau;
  double grad_clip;       /* < 0: no clipping (grad_clip None) */
  double policy_noise, noise_clamp; /* TD3 target smoothing (src/agent.py:174-179) */
  double actor_lr, actor_lr_min, critic_lr, critic_lr_min, alpha_lr;
  int64_t ac_scheduler_steps, cr_scheduler_steps;
  double alpha_min_steps; /* SACAgentConfig.alpha_min_steps is a float (src/utils.py:39) */
  int32_t device;
  int32_t use_graph;      /* 0: plain launches; 1: replay the step as a hipGraph where that pays (not on the
                             3-7-launch row-block path, measured faster issued one by one); 2: always */
  uint64_t seed;          /* device RNG for TD3 noise / SAC eps when not injected */
  int32_t pipeline_steps; /* DDPG: 0 = one launch per layer and phase after phase; 1 = co-schedule the
                             actor phase of step i with the critic phase of step i+1 in
                             gcrl_agent_update_n (they are independent: the critic phase reads the
                             TARGET actor; same arithmetic, fewer launches); 2 = additionally run
                             each phase's forward / input-gradient chain as ONE row-block launch
                             (csrc/rowchain.h; needs hidden_dim % 4 == 0, else falls back to 1) */
  int32_t n_quantiles;    /* TQC only; > 1 selects the DISTRIBUTIONAL variant of BASELINE.json configs[3] ("25 quantiles x 2
                             critics"): every critic outputs n_quantiles atoms, the num_critics*n_quantiles (<= 64) pooled target
                             atoms are sorted in one wavefront, the top top_drop PER CRITIC dropped, quantile-Huber loss.  NOT the
                             reference's TQC (scalar-critic ensemble): no reference parity, pinned to its oracle restatement.
                             0 / 1: the reference's semantics */
} gcrl_agent_config;

gcrl_agent* gcrl_agent_create(const gcrl_agent_config* cfg);

/* Measurement (bench.py's roofline leg): while enabled, gcrl_agent_update_n issues the row-block
 * DDPG step (pipeline_steps = 2) as plain launches instead of graph replays and brackets every
 * overlapped row-block launch (actor phase of step i || critic phase of step i+1) with two hipEvents
 * on its stream and a device wall-clock stamp pair.  _read waits for the pending events and returns
 * the launches since enabling, their summed hipEvent time (ms, includes the dispatch overhead of a
 * bracketed launch) and their summed in-kernel time (last block end - first block start, the
 * duration rocprofv3 reports).  Results are unchanged; only the issue path differs. */
int gcrl_agent_profile_enable(gcrl_agent* a, int on);
int gcrl_agent_profile_read(gcrl_agent* a, int64_t* launches_out, double* total_ms_out,
                            double* device_clock_ms_out);
void gcrl_agent_destroy(gcrl_agent* a);
void* gcrl_agent_stream(const gcrl_agent* a);

/* Networks are addressed by name: "actor", "target_actor", "critic_<i>", "target_critic_<i>"
 * (i from 0), "log_alpha".  A network's parameters are ONE flat fp32 vector in
 * torch `module.parameters()` order (weight [out,in] row-major, then bias, per layer; SAC
 * actor: Linear w,b, BatchNorm w,b per block, then mean_head, log_std_head — src/model.py),
 * so state_dict tensors are contiguous slices of it.  Buffers "bn_running_mean"/
 * "bn_running_var" are separate named vectors [L*H]. */
int64_t gcrl_agent_numel(const gcrl_agent* a, const char* name); /* <0: unknown name */
int gcrl_agent_get(gcrl_agent* a, const char* name, float* dst_host, int64_t n);
int gcrl_agent_set(gcrl_agent* a, const char* name, const float* src_host, int64_t n);
/* gradient of the last update() for "actor" / "critic_<i>" (pre-clip), optimiser moments
 * "adam_m:<net>" / "adam_v:<net>" — through the same get call. */

/* Xavier-uniform weights, bias 0.01 (src/model.py:39-42), targets hard-copied
 * (src/agent.py:1257-1258); device RNG seeded from cfg->seed.  Statistically, not bitwise,
 * equal to torch's initialisation: parity tests load explicit parameters with gcrl_agent_set.
 * Also what reset() does (src/agent.py:1461-1465): Linear layers only; optimiser moments,
 * schedulers and BN statistics are kept. `recreate_alpha` = SAC/TQC reset (src/agent.py:767). */
int gcrl_agent_init_weights(gcrl_agent* a, uint64_t seed, int recreate_alpha);
/* update_target_network(hard_update=True) */
int gcrl_agent_hard_update_targets(gcrl_agent* a);

/* update_target_network(hard_update=False, tau): every target <- tau*net + (1-tau)*target
 * (src/agent.py:1259-1271, :117-132, :487-496, :888-895) */
int gcrl_agent_soft_update_targets(gcrl_agent* a, double tau, void* stream);
/* Full resume state of the agent (extension): parameters and targets, Adam moments, BatchNorm running
 * statistics, alpha, optimiser step counts and scheduler positions, device-RNG counter.  One host blob of
 * gcrl_agent_state_size() bytes; loads only into an agent of the same shape. */
int64_t gcrl_agent_state_size(const gcrl_agent* a);
int gcrl_agent_save_state(gcrl_agent* a, void* dst_host, int64_t nbytes);
int gcrl_agent_load_state(gcrl_agent* a, const void* src_host, int64_t nbytes);

/* Optional injected inputs for one update (parity tests; all device pointers, may be NULL). */
typedef struct gcrl_update_inputs {
  const float* s_dev;   int32_t ld_s;    /* [B, S]  explicit batch instead of sampling */
  const float* a_dev;   int32_t ld_a;
  const float* r_dev;
  const float* ns_dev;  int32_t ld_ns;
  const float* d_dev;
  const float* noise_dev;      /* TD3: randn_like(action) [B, A]   (src/agent.py:175) */
  const float* eps_next_dev;   /* SAC/TQC: rsample eps for actor.sample(next_state) [B, A] */
  const float* eps_cur_dev;    /* SAC/TQC: rsample eps for actor.sample(states)     [B, A] */
  /* prioritised replay (PERBuffer, src/buffer.py:38-89): the caller draws the batch (np.random.choice over the priorities,
   * host) and passes the logical row indices and the importance-sampling weights; the critic losses become
   * (weights * loss).mean() (src/agent.py:193-197, :577-581, :993-997, :1320-1325).  Layer-per-launch schedule only
   * (pipeline_steps = 0).  The per-sample |td| of the step is the named vector "td_abs" (gcrl_agent_get). */
  const uint32_t* idx_host;    /* [B] logical ring indices instead of a random.sample draw (needs `her`) */
  const float* weights_host;   /* [B] */
} gcrl_update_inputs;

/* One agent.update(step).  Batch: sampled from `her` (HERBuffer.sample semantics) unless
 * inputs->s_dev is given.  Asynchronous: returns after enqueueing.  Returns the length of the
 * reference's return tuple for this step (DDPG 6/4, TD3 8/6, SAC & TQC 9/6 — the caller
 * dispatches on it, src/env.py:448-506) or a negative status.  `ticket_out` identifies the
 * metrics slot of this step. */
int gcrl_agent_update(gcrl_agent* a, gcrl_her* her, int64_t step,
                      const gcrl_update_inputs* inputs, int64_t* ticket_out, void* stream);
/* `n` consecutive updates step0..step0+n-1 (the loop of src/env.py:384-385; the buffer is not
 * mutated inside it, so all n batches are drawn and gathered by ONE gather launch).
 * tickets_out[n], tuple_len_out[n] optional. */
int gcrl_agent_update_n(gcrl_agent* a, gcrl_her* her, int64_t step0, int n,
                        int64_t* tickets_out, int32_t* tuple_len_out, void* stream);
/* DDPG, TD3 and SAC populations: `members` (1..16) independent agents of one kind (DDPG, TD3 or SAC) and equal shapes whose update steps
 * share launches.  Members must share kind, obs_dim, ac_dim, hidden_dim, layer_count, batch_size, num_critics, gradient_step, ac_update_freq,
 * polyak_every, pipeline_steps (2: the row-chain step), use_graph (0 or 1) and device; they may differ in seed, gamma, tau,
 * grad_clip and the learning-rate schedules.  A refusal names the field and happens before any device work.  TD3 populations run
 * batch_size < 2048 below the role-split critic phase (at most 255 row blocks, i.e. batch_size <= 1020); other TD3 configurations
 * are refused naming batch_size.  SAC populations run the path of the twin-critic SAC step at batch_size <= 512: the BatchNorm slab
 * launches, the role-split chain launches and the actor's heads folded into them (hidden_dim % 16 == 0, ac_dim <= 16, num_critics 2,
 * pipeline_steps 2); anything else is refused naming batch_size, hidden_dim, num_critics, pipeline_steps, or the environment switch
 * (GCRL_NO_BN_SLAB, GCRL_NO_SPLIT_ROLES, GCRL_NO_HEADS_FOLD) that takes the path away.  These two entries refuse TQC (kind: "TQC
 * populations are not implemented" by them): TQC populations are created with gcrl_pop_create_layered below.
 * alpha_lr and alpha_min_steps may differ between SAC members like the other rates.
 * gcrl_pop_create promises each member bit for bit a standalone agent, whatever launch forms that agent runs; a SAC population can only
 * promise that against an agent running the same forms (gcrl_pop_forms below), so gcrl_pop_create refuses SAC naming kind and
 * gcrl_pop_create_forms — the same entry for a caller that accepts the qualified guarantee — admits DDPG, TD3 and SAC.
 * gcrl_pop_create_layered: a population of TQC agents, whose step runs the layer-per-launch schedule (one launch per layer and
 * direction, the BatchNorm actor's slab launches), not the row chain.  Its guarantee is gcrl_pop_create_forms': each member is bit for
 * bit a standalone TQC agent running the forms gcrl_pop_forms reports (only bit 1, the row-split slab launches, exists on this schedule:
 * want[1] = want[2] = 0).  Admitted: kind TQC for every member (anything else is refused naming kind), n_quantiles <= 1 (the
 * distributional variant: n_quantiles), num_critics 2..8 and shared (num_critics), batch_size <= 512 and hidden_dim % 16 == 0 with the
 * slab launches on (batch_size, hidden_dim, GCRL_NO_BN_SLAB), use_graph 0 or 1, and the shared fields above; pipeline_steps is whatever a
 * standalone TQC agent is given (it never selects the row chain for this kind).  top_drop, alpha_lr and alpha_min_steps may differ between
 * members.  The members act through gcrl_pop_observe_act_bn.
 * gcrl_pop_member: member i as a full agent handle, owned by the population (every gcrl_agent_* entry works on it).
 * gcrl_pop_update_n: gcrl_agent_update_n(member i, rings[i], step0, n, ...) for every member, the members' launches of each
 * stage issued together; each member computes bit for bit what its own gcrl_agent_update_n computes.  Batches are drawn
 * from the rings in member order.  tickets_out / tuple_len_out: [members][n], optional.
 * gcrl_pop_forms: which launch forms with waits between workgroups the population's next update call runs, as bits of
 * gcrl_agent_get_meetings' result (1: row-split BatchNorm slab launches, 2: merged chain launch, 8: fused optimiser launch) — a form is
 * on when every member has it on, the device is this process's own and `members` times a member's workgroups of it are resident at
 * once.  Forms 2 and 8 compute the same bits as the launches that replace them.  Form 1 (SAC) sums a column's batch statistics in
 * another order than the one-workgroup slab launch: a SAC member is bit for bit a standalone agent RUNNING THE SAME FORMS (a
 * standalone agent's switches: GCRL_NO_BN_RSPLIT=1, GCRL_NO_RC_MERGE=1, GCRL_NO_OPT_FUSE=1).  Negative: an error code.
 * gcrl_pop_forms_terms: the two sides of the residency comparison, fixed at creation, for the forms of bits 1, 2 and 8 in this order:
 * want[3] = `members` times a member's workgroups of the form (0: the shape does not have it), capacity[3] = workgroups of the population
 * kernel resident at once (0: the device was shared or the occupancy query failed).  A population of two or more members runs form f when
 * 0 < want[f] <= capacity[f], every member has the form on and the device is not shared; a one-member population runs its member's forms.
 * GCRL_POP_NO_WAITS=1 in the environment at creation: the population admits no such form (A/B switch).
 * gcrl_pop_launch_counts: how the recorded launch positions of every gcrl_pop_update_n since creation were issued — `merged`: as one
 * launch of the kernel's population form for all members; `alone`: member by member (a launch without a population form, members
 * whose launches differ, or a one-member population).  Either pointer may be null.
 * The replay side of gcrl_pop_update_n: every member's indices are drawn first, in member order, then the members' gathers are
 * issued — as ONE launch of the gather kernel's population form (each member's own ring, indices or index generator, batch
 * matrices and control-block side copy; given the same indices bit for bit the members' own launches), or member by member.
 * rings[] may name one ring several times: those members draw from that ring's index stream in member order (device-RNG mode: the
 * ring's draw counter advances per member) and behave bit for bit like standalone agents sharing the ring, called in member order.
 * gcrl_pop_set_gather_merge: on != 0: the population gather launch; 0 (the state at creation): each member's own gather launch.
 * gcrl_pop_gather_counts: since creation — `calls`: update calls (one per chunk of at most the steps-per-call limit); `merged`:
 * population gather launches; `alone`: member-by-member gather launches (gcrl_pop_launch_counts does not count gathers).  Any
 * pointer may be null.
 *
 * The acting side of a population, one launch per call for all members (the trainer's loop, src/env.py:334-406, calls both per
 * vector-env step and per agent).  Every host array has a leading [members] dimension; each member computes bit for bit what its
 * own entry computes.  Refusals name the field and happen before any device work.  A one-member population hands the call to
 * the member's own entry.
 * gcrl_pop_observe_act: gcrl_agent_observe_act (src/env.py:348-355 + src/agent.py:1345-1366 / :253-270) of every member.
 * nz_obs[members] / nz_dg[members]: each member's normalisers (an entry, or the whole array, may be NULL: that part raw);
 * obs_host [members][n][obs_dim], dg_host [members][n][goal_dim], noise_host [members][n][A] float64 or NULL, out_host
 * [members][n][A] float64.  modes[i] is gcrl_agent_observe_act's mode of member i (0, 1, 2), or -1: the member is skipped — DDPG's
 * epsilon-random branch (src/agent.py:1348) involves no network and stays with the caller — and its out_host rows are left
 * untouched.  n <= batch_size.  Runs after every member's last update call and on its current weights.  Up to 32 rows per
 * member travel through a pinned, mapped block (one launch, no copy, no stream synchronisation); more rows take staged copies
 * around the same launch.  A SAC population is refused (GCRL_ERR_ARG, naming kind): a BatchNorm actor has no row-chain network;
 * its population acts through gcrl_pop_observe_act_bn (so does a TQC population).
 * gcrl_pop_observe_act_bn: the same for a population of BatchNorm actors (SAC, TQC): one launch of the population form of the members'
 * one-launch acting kernel, on each member's live parameter vector and running statistics.  eps_host [members][n][A] float64 is the
 * rsample eps of every member, or NULL: every member's deterministic action tanh(mean); there are no modes and no skipped members.
 * The other arrays, the row limits, the ordering after the members' update calls, the two forms (pinned block up to 32 rows per
 * member, staged copies beyond) and the counts are gcrl_pop_observe_act's.  Refused (GCRL_ERR_ARG, before any device work, out_host
 * untouched): a null handle or array, a population whose members are not BatchNorm actors (naming kind), n outside 1..batch_size,
 * obs_dim + goal_dim != state_dim, a member's normaliser of another size (naming the member).
 * gcrl_pop_process_step: gcrl_her_process_step_g (src/env.py:163-201, :167-175, :222-223) of every member's ring rings[i] with its
 * own normalisers: one launch stages all members' transitions, then each ring's episode flushes follow in member order (their
 * relabelling draws come from the rings' generators in that order).  The row arrays are those of gcrl_her_process_step_g, each
 * [members][n][.] (rewards_host, dones_host: [members][n]); ag_host is needed with a goal normaliser only.  rows_out[i] = what
 * member i's own gcrl_her_process_step_g returns.
 * gcrl_pop_acting_counts: calls of the two entries since creation and the kernel launches they issued for the network /
 * for the process-step stage (flush launches and a one-member population's own entries not counted); act_staged: how many of the
 * network launches took the staged form.  Any pointer may be null. */
typedef struct gcrl_pop gcrl_pop;
typedef struct gcrl_normalizer gcrl_normalizer;   /* (the device RunningNormalizer, declared below) */
gcrl_pop* gcrl_pop_create(const gcrl_agent_config* cfgs, int32_t members);
gcrl_pop* gcrl_pop_create_forms(const gcrl_agent_config* cfgs, int32_t members);
gcrl_pop* gcrl_pop_create_layered(const gcrl_agent_config* cfgs, int32_t members);
int gcrl_pop_member(gcrl_pop* p, int32_t i, gcrl_agent** out);
int32_t gcrl_pop_size(const gcrl_pop* p);
int gcrl_pop_update_n(gcrl_pop* p, gcrl_her* const* rings, int64_t step0, int32_t n, int64_t* tickets_out,
                      int32_t* tuple_len_out, void* stream);
int gcrl_pop_launch_counts(const gcrl_pop* p, int64_t* merged, int64_t* alone);
int gcrl_pop_set_gather_merge(gcrl_pop* p, int32_t on);
int gcrl_pop_gather_counts(const gcrl_pop* p, int64_t* calls, int64_t* merged, int64_t* alone);
int gcrl_pop_forms(gcrl_pop* p);
int gcrl_pop_forms_terms(const gcrl_pop* p, int64_t* want, int64_t* capacity);
int gcrl_pop_observe_act(gcrl_pop* p, gcrl_normalizer* const* nz_obs, gcrl_normalizer* const* nz_dg, const float* obs_host, int32_t obs_dim,
                         const float* dg_host, int32_t goal_dim, int32_t n, const double* noise_host, const int32_t* modes, double* out_host,
                         void* stream);
int gcrl_pop_observe_act_bn(gcrl_pop* p, gcrl_normalizer* const* nz_obs, gcrl_normalizer* const* nz_dg, const float* obs_host, int32_t obs_dim,
                            const float* dg_host, int32_t goal_dim, int32_t n, const double* eps_host, double* out_host, void* stream);
int gcrl_pop_process_step(gcrl_pop* p, gcrl_her* const* rings, gcrl_normalizer* const* nz_obs, int32_t update_stats, gcrl_normalizer* const* nz_dg,
                          int32_t update_goal_stats, const float* obs_host, const float* next_obs_host, int32_t obs_dim, const float* dg_host,
                          const float* next_dg_host, const float* ag_host, const float* next_ag_host, const float* actions_host,
                          const float* rewards_host, const uint8_t* dones_host, int32_t env0, int32_t n, int64_t* rows_out, void* stream);
int gcrl_pop_acting_counts(const gcrl_pop* p, int64_t* act_calls, int64_t* act_launches, int64_t* proc_calls, int64_t* proc_launches,
                           int64_t* act_staged);
void gcrl_pop_destroy(gcrl_pop* p);

/* Population-based training on a live population (extension: the reference's search driver prunes a trial and starts another,
 * src/param_search.py; here the slot is reused in place).  Refusals are GCRL_ERR_ARG, name the argument or field and happen before any
 * device work.
 * gcrl_pop_clone: for every pair k, member dst[k] receives member src[k]'s training state — ONE launch of pop_clone_kernel for all
 * pairs, no host synchronisation.  what & GCRL_CLONE_AGENT: everything gcrl_agent_save_state puts in its blob (parameters and targets,
 * Adam moments, BatchNorm running statistics, alpha, the optimiser step counts, the two current learning rates and the device-RNG
 * counter); afterwards gcrl_agent_save_state(dst) is byte for byte what gcrl_agent_load_state(dst, blob of src) leaves.  What the blob
 * does not carry — the configuration: gamma, tau, grad_clip, the schedules' base / minimum rates and lengths, alpha_lr,
 * alpha_min_steps, seed — stays the destination's own.  what & GCRL_CLONE_RING: rings[members] are the members' replay rings (as
 * gcrl_pop_update_n takes them; NULL without this bit): rows (the filled part, in logical order from physical row 0), staged partial
 * episodes, length and counters, bit for bit what gcrl_her_save_state / gcrl_her_load_state leave; rings of another capacity or
 * record layout are refused naming the field.  The launch is ordered after the last update call of every member involved; it then
 * closes the work of every member involved — sources too — with the event that closes an update call, so a destination's next
 * update / acting / get call, and a source's next write, are ordered after the launch on whatever stream they run (ring work: by
 * `stream`, the stream of the rings' pushes).  No host synchronisation once the segment table of a call is on the device: tables are
 * cached by content like the other population tables, so a call with new content — new pairs, or with GCRL_CLONE_RING a ring whose
 * head or length moved, i.e. nearly every ring clone — uploads its table with one allocation and one blocking copy of a few KiB, and
 * every 64th distinct table frees the cache, which synchronises the device.  A
 * destination's derived state is invalidated as gcrl_agent_load_state does it.  Refused: an index out of range (src / dst), a member
 * that is both a source and a destination, a destination listed twice (dst), pairs outside 1..16, an unknown or empty mask (what).  One
 * source may serve several destinations.
 * gcrl_agent_set_hparams: between update calls, the fields population members may differ in.  From the next step on the agent computes
 * bit for bit what an agent CONSTRUCTED with these values computes from the same state (parameters, moments, step counts, RNG
 * position).  Scheduler positions are kept: the two current rates become the new schedules evaluated at the kept positions
 * (csrc/lr_sched.cc, the recursion replayed from the new base rate: O(steps taken) host work).  Works on a standalone agent and on a
 * population member; no launch form changes.  alpha_lr / alpha_min_steps are read for SAC / TQC only.  The creating entries validate
 * none of these fields, so only what cannot be stepped with is refused, naming the field: a value that is not a number, a learning
 * rate that is not finite and > 0, a negative minimum, a scheduler length < 1 (grad_clip < 0: no clipping).
 * gcrl_pop_replace: member i becomes what the creating entry would have made of *cfg in that slot: weights from cfg->seed, targets
 * hard-copied, moments, step counts and scheduler positions zero, BatchNorm statistics and log_alpha initial, device RNG re-keyed.  cfg
 * must agree with the population in every shared field, and its rates must be what gcrl_agent_set_hparams accepts (refused naming the
 * field, member i untouched).  Nothing of the agent is reallocated (the member's replay ring is the caller's: src/population.py); the
 * other members, the device tables and admission are unaffected; captured graphs of the member are dropped.  Synchronises the device
 * (it uploads the initial weights from the host). */
#define GCRL_CLONE_AGENT 1u
#define GCRL_CLONE_RING 2u
typedef struct gcrl_hparams {
  double actor_lr, actor_lr_min, critic_lr, critic_lr_min;
  int64_t ac_scheduler_steps, cr_scheduler_steps;
  double gamma, tau;
  double grad_clip;       /* < 0: no clipping */
  double alpha_lr, alpha_min_steps;   /* SAC / TQC */
} gcrl_hparams;
int gcrl_pop_clone(gcrl_pop* p, gcrl_her* const* rings, const int32_t* src, const int32_t* dst, int32_t pairs, uint32_t what, void* stream);
int gcrl_agent_set_hparams(gcrl_agent* a, const gcrl_hparams* h);
int gcrl_pop_replace(gcrl_pop* p, int32_t i, const gcrl_agent_config* cfg);
/* Metrics of a ticket, in the reference's tuple order, as fp32 (waits for that step only).
 * n = tuple length returned by the update. */
int gcrl_agent_metrics(gcrl_agent* a, int64_t ticket, double* out_host, int n);

/* Data-parallel hooks: the step is split at the two gradient exchanges.
 * phase 0: sample + critic fwd/bwd  -> caller all-reduces grads of "critic_*"
 * phase 1: critic clip/optimiser/Polyak + actor fwd/bwd -> caller all-reduces "actor" grads
 * phase 2: actor clip/optimiser (+alpha, + actor Polyak)
 * gcrl_agent_grad_ptr returns the device pointer + numel of the flat gradient block of the
 * phase (all critics contiguous / actor (+log_alpha grad)). `grad_scale` multiplies the
 * gradients before clipping (1/world after an all-reduce sum). */
int gcrl_agent_update_phase(gcrl_agent* a, gcrl_her* her, int64_t step, int phase,
                            const gcrl_update_inputs* inputs, float grad_scale,
                            int64_t* ticket_out, void* stream);
int gcrl_agent_grad_ptr(gcrl_agent* a, int phase, float** ptr_dev_out, int64_t* numel_out);
/* Data-parallel trainer cycle: plan n steps at once — one index upload and ONE gather launch for
 * all n batches, as gcrl_agent_update_n does — then run step i's phases 0,1,2 in order with the
 * caller's two gradient all-reduces in between; gcrl_agent_dp_end closes the cycle. */
int gcrl_agent_dp_begin(gcrl_agent* a, gcrl_her* her, int64_t step0, int n, float grad_scale,
                        int64_t* tickets_out, int32_t* tuple_len_out, void* stream);
int gcrl_agent_dp_phase(gcrl_agent* a, int i, int phase, void* stream);
int gcrl_agent_dp_end(gcrl_agent* a, void* stream);
/* Engine-scheduled form of the same cycle: after gcrl_agent_dp_begin, call gcrl_agent_dp_run
 * repeatedly.  Each call enqueues the next segment of the cycle and names the gradient block the
 * caller must all-reduce (sum over ranks) before the next call (*reduce_numel_out == 0: nothing to
 * exchange).  Returns 1 while segments remain, 0 when the cycle is complete (it is then closed),
 * negative on error.  The engine picks the schedule: three phases per step in general; for runs
 * of plain DDPG steps the software-pipelined form, where the critic gradients of step i+1 and the
 * actor gradients of step i are adjacent in memory and travel in ONE all-reduce per step. */
int gcrl_agent_dp_run(gcrl_agent* a, float** reduce_ptr_out, int64_t* reduce_numel_out, void* stream);
/* In-engine gradient exchange: an RCCL communicator owned by the library (one process per GPU; RCCL is bound at
 * run time from `rccl_path` — the librccl the host process already uses — or the default soname when NULL).
 * Rank 0 makes the 128-byte id and hands it to the other ranks by any side channel (torch.distributed's store,
 * MPI, a file).  New design: the reference has no distributed code. */
typedef struct gcrl_dp gcrl_dp;
int gcrl_dp_unique_id(uint8_t* id128_out, const char* rccl_path);
gcrl_dp* gcrl_dp_create(int rank, int world, const uint8_t* id128, int device, const char* rccl_path);
void gcrl_dp_destroy(gcrl_dp* d);
int gcrl_dp_world(const gcrl_dp* d);
int gcrl_dp_allreduce_sum(gcrl_dp* d, float* buf_dev, int64_t n, void* stream); /* in place, fp32 */
int gcrl_dp_broadcast(gcrl_dp* d, float* buf_dev, int64_t n, int root, void* stream);
/* Test hook of the replay ring's deque(maxlen) bookkeeping (csrc/ring_book.h; what collections.deque(maxlen=max_len) does for
 * the reference's buffers, src/buffer.py:95, :8-20).  Host-only: for append i of `appends[0..n)` rows to a ring of `capacity`
 * rows (initially `len0` rows, head `head0`) reports the physical row its first row goes to and how many of its rows are
 * overwritten inside the same append; returns the final head / len. */
int gcrl_ringbook_sim(int64_t capacity, int64_t head0, int64_t len0, const int64_t* appends, int n, int64_t* tail_out, int64_t* skip_out,
                      int64_t* head_out, int64_t* len_out);
/* ------------------------------------------------------------------------------------------
 * The gradient exchange INSIDE the engine's launch sequence (csrc/xchg_ipc.hip; round 4).  New design: the reference is
 * single-process, BASELINE.json's north star asks for the all-reduce of actor/critic gradients over xGMI.  One process per GPU of
 * ONE node (world <= 8); every rank's gradient arena is mapped by every peer through HIP IPC handles and one kernel per exchange
 * performs a two-shot all-reduce peer to peer: the owner of a 1024-float chunk (chunk c: rank c mod world) adds the chunk of
 * every rank in RANK ORDER (bitwise identical replicas), forms its sum of squares, and writes both back to every rank in
 * place (into a fine-grained receive buffer of the arena's layout: gcrl_xchg_read) — the optimiser launch reads the reduced
 * gradients and the clip norm's partials, no separate norm launch, and the
 * exchange is a plain kernel node: hipGraph replay, control-advance riders and multi-step graphs stay on.
 *   gcrl_xchg_create    over an arena (a hipMalloc base pointer, 16-byte aligned) cut into `nseg` segments (offset / length in
 *                       floats: the nets); every rank must pass the same layout
 *   gcrl_xchg_handles   this rank's record (GCRL_XCHG_HANDLE_BYTES) for the peers; gather the records of all ranks in rank
 *                       order (torch.distributed's store / all_gather) and pass them to gcrl_xchg_connect on every rank
 *   gcrl_xchg_allreduce in-place sum over the ranks of segments [seg0, seg0 + nseg), stream-ordered; EVERY rank must enqueue
 *                       the same sequence of exchanges.  Waits are bounded (~1 s): a rank that never arrives leaves NaN and
 *                       a status bit that the owner's next synchronising call reports (GCRL_ERR_STATE)
 *   gcrl_agent_xchg_create / gcrl_agent_set_exchange   the same over an agent's own gradient arena (segments: every critic, the
 *                       actor, log_alpha), and attaching it: from then on EVERY update entry point (gcrl_agent_update,
 *                       _update_n, _update_phase) exchanges the critic gradients after the critic backward and the actor
 *                       (+ log_alpha) gradients after the actor backward — one exchange per overlapped DDPG step — and scales
 *                       by 1 / world inside the optimiser launches.  Reference semantics kept: the actor loss goes through the
 *                       STEPPED critic (src/agent.py:1389-1401, :548-639).  NULL detaches.
 * xGMI time is unmeasured (1-GPU boxes); world-size-1 cost: profiles/r04_dp_overhead_world1.json. */
#define GCRL_XCHG_HANDLE_BYTES 256
typedef struct gcrl_xchg gcrl_xchg;
gcrl_xchg* gcrl_xchg_create(float* arena_dev, int64_t arena_floats, const int64_t* seg_off, const int64_t* seg_n, int nseg, int rank,
                            int world, int device);
void gcrl_xchg_destroy(gcrl_xchg* x);
int gcrl_xchg_handles(gcrl_xchg* x, uint8_t* out, int64_t n);
int gcrl_xchg_connect(gcrl_xchg* x, const uint8_t* all_ranks_records, int64_t n);
int gcrl_xchg_world(const gcrl_xchg* x);
int gcrl_xchg_allreduce(gcrl_xchg* x, int seg0, int nseg, void* stream);
/* sums of squares of segment `seg`'s reduced 1024-float chunks as the last exchange left them (what the optimiser launch sums
 * for the clip norm); returns how many (synchronises the device; tests) */
int gcrl_xchg_get_partials(gcrl_xchg* x, int seg, float* out_host, int n);
/* the reduced values of [first, first + n) arena floats as the last exchange left them, to the host (synchronises; tests) */
int gcrl_xchg_read(gcrl_xchg* x, int64_t first, int64_t n, float* out_host);
/* collective self-test after gcrl_xchg_connect (every rank calls it): exchanges a known pattern through segment 0 and checks
 * the sum; GCRL_ERR_STATE when a peer's mapping, layout or arrival is wrong — the host side then falls back to another exchange
 * before training starts (src/dp.py).  Leaves the arena as it found it. */
int gcrl_xchg_selftest(gcrl_xchg* x, void* stream);
int gcrl_xchg_reset(gcrl_xchg* x);   /* counters back to zero after a reported failure (call on every rank, ranks synchronised around it) */
gcrl_xchg* gcrl_agent_xchg_create(gcrl_agent* a, int rank, int world);
int gcrl_agent_set_exchange(gcrl_agent* a, gcrl_xchg* x);
/* The whole data-parallel trainer cycle begun by gcrl_agent_dp_begin as ONE host call: every segment of the
 * engine's schedule and, after each, the all-reduce(sum) of the gradient block it names, all enqueued on `stream`
 * (what the caller of gcrl_agent_dp_run does one Python round trip at a time). */
int gcrl_agent_dp_run_all(gcrl_agent* a, gcrl_dp* d, void* stream);
/* SyncBN for the data-parallel BatchNorm actors (SACAgent / TQCAgent; new design — torch's SyncBatchNorm is what a DDP port
 * of src/model.py:100-108 would use).  After this call the batch statistics of every BatchNorm1d forward and backward are
 * those of the CONCATENATED batch of all `world` ranks (rank r's rows = rows [r*B, (r+1)*B) of it), so that G ranks x B rows
 * equal 1 rank x G*B rows for these agents as well: per BatchNorm layer and pass the ranks' row-block partials
 * (2 * world * ceil(B/64) * H floats) are summed over the ranks — by the library-owned communicator `dp` when given, else by
 * `fn` (an in-place all-reduce(sum) of n device floats, stream-ordered on `stream` or synchronous; returns 0) — and merged in
 * the order a single process with the big batch uses.  dgamma / dbeta stay each rank's share (the gradient exchange sums
 * them).  Steps then run as plain launches (no hipGraph replay).  Call it before the first update; world = 1 switches it off. */
typedef int (*gcrl_exchange_fn)(float* buf_dev, int64_t n, void* stream, void* user);
int gcrl_agent_dp_sync_bn(gcrl_agent* a, int world, int rank, gcrl_dp* dp, gcrl_exchange_fn fn, void* user);
/* The same with the partials exchanged by the in-engine peer-to-peer kernel (round 5): gcrl_agent_bn_xchg_create allocates the
 * partials' arena and returns an exchange handle over it (connect it like the gradient exchange: gcrl_xchg_handles / _connect /
 * _selftest; the caller owns it and destroys it after switching SyncBN off); gcrl_agent_dp_sync_bn_xchg switches SyncBN on
 * through it.  The exchange is then a kernel of the step's launch sequence: hipGraph replay and multi-step graphs stay on.
 * New design (the reference is single-process, src/model.py:107 BatchNorm1d on one batch). */
gcrl_xchg* gcrl_agent_bn_xchg_create(gcrl_agent* a, int rank, int world);
int gcrl_agent_dp_sync_bn_xchg(gcrl_agent* a, int world, int rank, gcrl_xchg* bx);
/* Launches whose workgroups WAIT for each other inside the kernel (csrc/meet.h: the row groups of a BatchNorm slab, the role
 * workgroups of a twin-critic row block) are admitted only when every workgroup of the launch is resident at once — judged by
 * the kernel's occupancy on a device this process has to itself.  New design (the reference is eager PyTorch: no such forms).
 *   gcrl_set_shared_device(1)   process-wide (also GCRL_SHARED_GPU=1 in the environment, read at first use): the device is
 *                               shared with other processes / streams that hold CUs (several ranks on one GPU, another
 *                               library's collectives) — handles created afterwards use the launch forms without waits;
 *   gcrl_agent_set_meetings     switches an existing handle (0: off; 1: on where admissible); captured graphs are dropped;
 *                               returns a bit mask of the forms now active (1 slab row groups, 2 row-chain roles: merged phases,
 *                               DDPG's two-role critic phase; 4 reserved, always 0 (a launch form deleted in round 18); 8 the
 *                               fused dW | db + clip + optimiser launch of the row-chain agents, csrc/dw_adam.hip — the reference's
 *                               backward -> clip_grad_norm_ -> optimizer.step(), src/agent.py:1326-1333, :1288-1300, :199-222);
 *   gcrl_agent_get_meetings     the same mask, changing nothing;
 *   a wait that times out (~1 s) poisons that launch's statistics / gradients with NaN AND is reported: the next call that
 *   synchronises the handle (gcrl_agent_metrics, _get, _save_state) returns GCRL_ERR_STATE once, after which the handle works
 *   again — the reference raises on any failed step (src/agent.py:659-699);
 *   gcrl_agent_debug_meet_fault injects such a failure into the handle's next launch (tests). */
int gcrl_set_shared_device(int shared);
int gcrl_agent_set_meetings(gcrl_agent* a, int on);
int gcrl_agent_get_meetings(gcrl_agent* a);
int gcrl_agent_debug_meet_fault(gcrl_agent* a);
/* Which of the handle's fused DDPG row-chain launches read the backward chains' act' multipliers from LDS instead of the global
 * saves (csrc/rowchain.h rowchain_lds_mul_ok: the form fits the LDS and costs no resident workgroup; GCRL_RC_GLOBAL_MUL=1 at
 * creation: none).  Bits: 1 a launch of critic-phase workgroups only, 2 of actor-phase workgroups only, 4 the overlapped launch of
 * both; 0 also when no launch of the handle goes through that kernel (SAC, TQC).  Same results either way; changes nothing.
 * New design (the reference is eager PyTorch: no such forms). */
int gcrl_agent_rowchain_form(gcrl_agent* a);
/* 1 when the handle's fused DDPG row-chain launches take the stream form of their chained layer passes (csrc/rowchain.h WStream: the
 * first stage of a pass's weight rows is requested by the pass before it; plain DDPG at 4 rows per workgroup, hidden width <= 256, two
 * hidden layers or more), 0 otherwise (GCRL_RC_NO_STREAM=1 at creation, another shape, or an agent without that launch).  Same bits
 * either way; changes nothing.  New design (the reference is eager PyTorch: no such forms). */
int gcrl_agent_rowchain_stream(gcrl_agent* a);
/* Number of L2-warming rider workgroups the handle's overlapped fused DDPG row-chain launch carries behind its role workgroups
 * (csrc/rowchain.hip rc_warm_rider: workgroups on otherwise idle CUs that only load, and discard, the weight matrices the roles are
 * about to stream, so that each XCD's L2 holds them at first use); 0 when the launch has none (GCRL_RC_NO_WARM=1 at creation, a launch
 * that does not take the stream form, no idle CUs left, or an agent without that launch).  Riders store nothing: same bits either way;
 * changes nothing.  New design (the reference is eager PyTorch: no such forms). */
int gcrl_agent_rowchain_warm(gcrl_agent* a);
/* The launch rules gcrl_agent_create settled for this handle, as they stand now (tests name the form they ran on): out[0..n) in this
 * order, as many as n holds (at most 10) — rows per row-chain workgroup (4, 8 or 16), row chain (else the layer-per-launch schedule),
 * split_roles (SAC: role-parallel chain launches), rc_merge (those merged into one launch), split_k (TD3: role-parallel critic phase),
 * rc_merge_k (its two launches as one), ddpg_ksplit (DDPG: two-role critic phase), opt_fuse (fused dW + optimiser launch), bn_slab
 * (SAC: BatchNorm slab launches), bn_rsplit (row groups per slab: 1 or 4).  Returns the number of fields written; reads the handle
 * only: no kernel, launch or rule changes.  New design (the reference is eager PyTorch: no such forms). */
int gcrl_agent_update_forms(gcrl_agent* a, int32_t* out, int n);
/* device pointer of a named vector (parameters / grads), for zero-copy interop */
int gcrl_agent_dev_ptr(gcrl_agent* a, const char* name, float** ptr_dev_out, int64_t* numel_out);

/* Batched actor inference for select_action (src/agent.py:1345-1366, :641-647): obs_dev
 * [n, S] -> out_dev [n, A]: DDPG/TD3 the network output (already tanh, src/model.py:24);
 * SAC/TQC tanh(mean) in eval mode (BatchNorm running statistics) when eps_dev is NULL,
 * else tanh(mean + std*eps). */
int gcrl_agent_act(gcrl_agent* a, const float* obs_dev, int n, int ld_obs, float* out_dev,
                   int ld_out, const float* eps_dev, void* stream);
/* The same from and to HOST arrays (n <= batch_size rows): staging, both copies and the stream
 * synchronisation happen inside; what select_action needs per vector-env step in one call. */
int gcrl_agent_act_host(gcrl_agent* a, const float* obs_host, int n, int ld_obs, float* out_host,
                        int ld_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The acting side: RunningNormalizer on the device (src/utils.py:68-98: float32 batch moments in
 * numpy's order, float64 parallel-variance merge, clip to +-clip_range) and the two fused entry points of one
 * vector-env step.  Rows are float32, `ld` floats apart; `on_device` says where they live.
 * ---------------------------------------------------------------------------------------- */
typedef struct gcrl_normalizer gcrl_normalizer;
gcrl_normalizer* gcrl_normalizer_create(int size, double clip_range, double eps, int device);   /* __init__ :69-73 */
void gcrl_normalizer_destroy(gcrl_normalizer* z);
int gcrl_normalizer_size(const gcrl_normalizer* z);
int gcrl_normalizer_update(gcrl_normalizer* z, const float* x, int n, int ld, int on_device, void* stream);   /* update :75-81 */
/* normalize :95-97, result cast to float32 (what the trainer's torch.from_numpy(..).float() does, src/env.py:189-190) */
int gcrl_normalizer_normalize(gcrl_normalizer* z, const float* x, int n, int ld, int on_device, float* out, int ld_out,
                              int out_on_device, void* stream);
int gcrl_normalizer_get(gcrl_normalizer* z, double* mean_host, double* var_host, double* count_host);   /* save :99-108 */
int gcrl_normalizer_set(gcrl_normalizer* z, const double* mean_host, const double* var_host, double count, double clip_range);
/* The reference's `RunningNormalizer.load` (src/utils.py:108-117) brings mean / var back as FLOAT32 arrays, and everything it
 * computes afterwards — normalize and the merge of update — then runs in float32 (only the count stays a Python float).  `on`
 * != 0 puts the handle in that regime (the statistics set before should be float32 values); pinned by
 * tests/golden/normalizer_loaded.npz.  A created normaliser starts in the float64 regime. */
int gcrl_normalizer_set_float32(gcrl_normalizer* z, int on);
int gcrl_normalizer_is_float32(const gcrl_normalizer* z);
/* The dtype of the rows the REFERENCE's trainer would pass decides numpy's arithmetic.  Observation batches are float64
 * arrays there (the vector env allocates them with the observation space's dtype, which TimeFeatureWrapper declares float64,
 * src/utils.py:156; the values inside are float32-valued, so the float32 rows of this ABI carry them exactly), goal batches
 * float32.  `on` != 0: treat the rows of every later update / normalize / fused entry as float64 — batch moments, merge,
 * subtraction and division in float64 (`self.var * self.count` and sqrt(var) + 1e-8 of a LOADED normaliser stay float32 values),
 * and the first update after a load turns the statistics back into float64 (gcrl_normalizer_is_float32 then reports 0).
 * Pinned by tests/golden/normalizer_f64.npz.  Default off (float32 rows: normalizer.npz, normalizer_loaded.npz). */
int gcrl_normalizer_set_rows_float64(gcrl_normalizer* z, int on);
/* select_action for one vector-env step from RAW host rows (src/env.py:348-355 + src/agent.py:1345-1366 / :253-270 /
 * :641-647): normalize_state_batch with the given normalisers (NULL: that part raw), actor, post-processing —
 * mode 0: clip(tanh(net), -1, 1); 1: clip(tanh(net) + noise, -1, 1), noise = np.random.normal draws [n, A] float64;
 * 2: the network output as it is.  SAC / TQC ignore `mode`: noise = rsample eps (NULL: deterministic tanh(mean)).
 * out_host [n, A] float64.  DDPG's epsilon-random branch (:1348) stays with the caller (shared `random` stream). */
int gcrl_agent_observe_act(gcrl_agent* a, gcrl_normalizer* nz_obs, gcrl_normalizer* nz_dg, const float* obs_host, int obs_dim,
                           const float* dg_host, int goal_dim, int n, const double* noise_host, int mode, double* out_host,
                           void* stream);
/* How gcrl_agent_observe_act has done its work since the agent was created: calls, the kernel launches, the host <-> device
 * copies and the stream synchronisations it issued.  Up to the rows the kernel arguments hold (n * state_dim <= 640, n * action_dim
 * <= 96) every agent kind takes ONE launch, no copy and no synchronisation per call: DDPG / TD3 the row-chain act kernel
 * (src/model.py:32-49 + src/agent.py:1345-1366 / :253-270), SAC / TQC the BatchNorm actor's (src/model.py:118-141 in eval mode +
 * src/agent.py:641-647); more rows: copies up, the same launch, a copy down, one synchronisation.  GCRL_ACT_STAGED=1 in the
 * environment selects the staged forms (SAC / TQC: the chain of separate launches: normalisers, a GEMM and a BatchNorm launch per
 * hidden block, the heads, the sampling, the float64 conversion).  A launch that rebuilds weight copies after a parameter write is
 * counted with the call that issued it.  Copies and synchronisations are counted where they are issued, and so are the launches of
 * the one-launch forms; the launches of the staged chain (gcrl_agent_act's part) and of a weight-copy rebuild are declared from
 * those functions' definitions.  Refuses a NULL handle; any of the four pointers may be NULL. */
int gcrl_agent_acting_counts(const gcrl_agent* a, int64_t* calls, int64_t* launches, int64_t* copies, int64_t* syncs);
/* _process_step for one vector-env step (src/env.py:163-201) from raw host rows: normaliser update with [obs ; next_obs]
 * (when update_stats), state = [normalize(obs) | dg], next_state = [normalize(next_obs) | next_dg] built on the device
 * from the UPDATED statistics, then the n pushes of gcrl_her_push_batch (achieved goal = next_ag, done = dones).
 * Goals are not normalised here; gcrl_her_process_step_g adds the goal normaliser (g_normalize = True, src/env.py:167-175,
 * :222-223): its update from [dg ; next_dg ; ag ; next_ag] (ag_host = the state's achieved goals, only for these statistics), then
 * the goal columns of both states and the pushed achieved goal normalised by the UPDATED goal statistics.  Returns ring rows appended. */
int64_t gcrl_her_process_step(gcrl_her* h, gcrl_normalizer* nz_obs, int update_stats, const float* obs_host,
                              const float* next_obs_host, int obs_dim, const float* dg_host, const float* next_dg_host,
                              const float* next_ag_host, const float* actions_host, const float* rewards_host,
                              const uint8_t* dones_host, int env0, int n, void* stream);
int64_t gcrl_her_process_step_g(gcrl_her* h, gcrl_normalizer* nz_obs, int update_stats, gcrl_normalizer* nz_dg, int update_goal_stats,
                                const float* obs_host, const float* next_obs_host, int obs_dim, const float* dg_host,
                                const float* next_dg_host, const float* ag_host, const float* next_ag_host, const float* actions_host,
                                const float* rewards_host, const uint8_t* dones_host, int env0, int n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stand-alone ops exposed for tests / reuse.
 * ---------------------------------------------------------------------------------------- */
/* Row-wise sort of `width` (<= 64) fp32 values per row in one wavefront (bitonic network via
 * cross-lane swaps), drop the `drop` largest, mean of the rest: the truncation of
 * src/agent.py:919-921 / :972-974 generalised to BASELINE.json's 25x2-atom shape.
 * in_dev [rows, width] -> sorted_dev [rows, width] (optional) , mean_dev [rows]. */
int gcrl_sort_truncate_mean(const float* in_dev, int64_t rows, int width, int drop,
                            float* sorted_dev, float* mean_dev, void* stream);

/* The batched fp32-MFMA GEMM every Linear forward/backward of the engine runs on, as a single
 * problem: C[M,N] = act(A.B + bias) with element strides (A(m,k) = A[m*a_rs + k*a_cs],
 * B(k,n) = B[k*b_rs + n*b_cs], C row stride c_rs); act: 0 none, 1 LeakyReLU(0.01), 2 ReLU,
 * 3 tanh.  shape: 0 auto, 1 = 16x16 tile per workgroup with K split over its 4 waves,
 * 2 = 16x16 per wave, 3 = 32x32 per wave, 4 = LDS-tiled 64x64 per workgroup, 5 = K == 1 only: the outer product as a
 * streaming kernel (16-byte aligned B / C / bias, N and c_rs multiples of 4, b_cs == 1; else GCRL_ERR_ARG) — tests sweep all. */
int gcrl_gemm_f32(const float* a_dev, int64_t a_rs, int64_t a_cs, const float* b_dev, int64_t b_rs,
                  int64_t b_cs, float* c_dev, int64_t c_rs, const float* bias_dev, int M, int N,
                  int K, int act, int shape, void* stream);

/* The weight / bias gradient of a Linear layer as the engine computes it at batch >= 1024 (csrc/gemm_tiled.h): dW [out, in] =
 * G^T X and db [out] = column sums of G, for G [batch, ldg] (first `out` columns) and X [batch, ldx] (first `in` columns), on
 * the LDS-tiled form with the reduction over the batch split over `ksplit` workgroups per 64x64 tile (1: no split) — partial
 * tiles through a scratch array, a ticket per tile, the last arriver sums them in index order (deterministic).  Stand-alone
 * for tests: allocates and frees its scratch per call (the engine keeps it per layer).  `sumsq_dev`, if not null, receives the
 * sum of squares of dW | db (one float), as the fused global-norm clip consumes it.  Reference: the backward of
 * `nn.Linear` (src/model.py:18,57,63). */
int gcrl_gemm_dw_split_f32(const float* g_dev, int64_t ldg, const float* x_dev, int64_t ldx, float* dw_dev, float* db_dev,
                           int out, int in, int batch, int ksplit, float* sumsq_dev, void* stream);

/* One problem of gcrl_gemm_batch_f32: everything the engine's problem record (csrc/gemm_mfma.h, GemmDesc) lets a caller choose.
 *   C[m*c_rs + n] = act(sum_k A(m,k) B(k,n) + bias[n]) * mul'(H[m*h_rs + n])      A(m,k) = a[m*a_rs + k*a_cs], B(k,n) = b[k*b_rs + n*b_cs]
 * act: 0 none, 1 LeakyReLU(0.01), 2 ReLU, 3 tanh.  mul: 0 none, 1 / 2 / 3 = the derivative of LeakyReLU / ReLU / tanh at the SAVED
 * activation H (h > 0 decides; 1 - h^2).  ones_col: B(k, N-1) := 1 and column N-1 of the result goes to col_out[m] instead of C (the
 * bias gradient of a dW | db problem; N >= 2).  slot_dev: if not null, a device word s; the operands are then a + s*a_slot,
 * b + s*b_slot, c + s*c_slot, h + s*h_slot (element strides), read on the device at launch time.  shape_hint: the problem's own tile
 * form (0: the launcher's rule); ksplit: the LDS-tiled form's reduction split (0 / 1: none).  bn_part_dev: per-row-tile (mean, M2)
 * of every column of C, [2 * ceil(M / T)][N] floats, T = 16 on form 1 and 64 on form 4.  sumsq_dev: one float, the sum of squares of
 * everything the problem wrote.  form_out: set by the call to the tile form (1..5) the problem ran on. */
typedef struct gcrl_gemm_problem {
  const float* a_dev; int64_t a_rs, a_cs;
  const float* b_dev; int64_t b_rs, b_cs;
  float* c_dev; int64_t c_rs;
  const float* bias_dev;
  const float* h_dev; int64_t h_rs;
  float* col_out_dev;
  int32_t M, N, K, act, mul, ones_col;
  const int32_t* slot_dev;
  int64_t a_slot, b_slot, c_slot, h_slot;
  int32_t shape_hint, ksplit;
  float* bn_part_dev;
  float* sumsq_dev;
  int32_t form_out, reserved;
} gcrl_gemm_problem;

/* The same GEMM with its whole problem record, 1..12 problems per call, exactly as the engine issues it per layer: one launch per tile
 * form present.  shape: 1..5 forces one form on every problem; 0 = each problem's own (shape_hint, else the launcher's rule).  The
 * call owns what the engine owns per layer: the split partials and a zeroed ticket array of every problem with ksplit > 1 (the batch
 * is then launched TWICE — the tickets must return to zero by themselves — and everything such a problem wrote is set to all-ones
 * words in between), the zero-filled sum-of-squares partials, sized from the launcher's own tile count, which are added on the host
 * in index order to one float.  It allocates, synchronises and frees per call: for tests, not a fast path.  The launcher's
 * refusals come back as GCRL_ERR_ARG with nothing written.  The kernels address an operand with 32-bit byte offsets: every operand
 * (last element's index + 1, slot offset included) must stay below 2 GiB. */
int gcrl_gemm_batch_f32(gcrl_gemm_problem* problems_host, int n, int shape, void* stream);

/* nn.BatchNorm1d in training mode followed by ReLU, as the SAC / TQC actors run it per hidden layer
 * (src/model.py:106-108: Linear -> BatchNorm1d -> ReLU; eps 1e-5, momentum 0.1, running variance unbiased), forward and
 * backward as single problems.  All pointers are device memory, row-major [B, H]; H must be a multiple of 4 and every
 * pointer 16-byte aligned.  `scratch_dev`: 2 * ceil(B/64) * H floats.
 *   fwd: z -> h = relu(gamma * xhat + beta); saves xhat [B,H] and invstd [H]; updates running_mean / running_var in place.
 *   bwd: dh (gradient w.r.t. h), xhat / invstd from the forward -> dz [B,H], dgamma [H], dbeta [H]. */
int gcrl_bn_relu_fwd_f32(const float* z_dev, int B, int H, const float* gamma_dev, const float* beta_dev, float* h_dev,
                         float* xhat_dev, float* invstd_dev, float* running_mean_dev, float* running_var_dev,
                         float* scratch_dev, void* stream);
int gcrl_bn_relu_bwd_f32(const float* dh_dev, const float* xhat_dev, const float* invstd_dev, const float* gamma_dev,
                         const float* beta_dev, int B, int H, float* dz_dev, float* dgamma_dev, float* dbeta_dev,
                         float* scratch_dev, void* stream);

/* [Linear -> BatchNorm1d(train) -> ReLU] (src/model.py:104-108) as ONE launch per direction (csrc/bn_slab.hip: a workgroup
 * owns 16 columns over all rows, so the batch statistics never leave it): what the SAC / TQC actors run per hidden layer at
 * B <= 512, H % 16 == 0 (anything else: GCRL_ERR_ARG; the engine then uses the GEMM + BatchNorm launches above).
 *   fwd: x [B, ldx] (first K columns), w [H, K], bias / gamma / beta [H] -> h = relu(bn(x w^T + bias)) [B, H]; xhat [B, H] and
 *        invstd [H] (either may be null); bstat [2][H] = the batch mean and the biased batch variance (the running statistics
 *        are updated from these by the step's tanh-Gaussian launch).
 *   bwd: dh = g_up [B, ldg] (first K_up columns) . w_up [K_up, H]  — the input gradient of the consuming Linear layer —
 *        -> dz written over xhat_dz [B, H] (xhat on entry), dgamma [H], dbeta [H].  ldg % 4 == 0, g_up 16-byte aligned.
 *   row_split > 1 (and B > 128): the rows of a slab split over ceil(B / 128) workgroups that exchange their column partials once
 *        per launch through agent-scope memory and a bounded wait (what the engine uses for its K >= 128 layers); <= 1: one
 *        workgroup per slab holds every row. */
int gcrl_bn_linear_slab_fwd_f32(const float* x_dev, int64_t ldx, const float* w_dev, const float* bias_dev,
                                const float* gamma_dev, const float* beta_dev, int B, int H, int K, float* h_dev,
                                float* xhat_dev, float* invstd_dev, float* bstat_dev, int row_split, void* stream);
int gcrl_bn_linear_slab_bwd_f32(const float* g_up_dev, int64_t ldg, int K_up, const float* w_up_dev, float* xhat_dz_dev,
                                const float* invstd_dev, const float* gamma_dev, const float* beta_dev, int B, int H,
                                float* dgamma_dev, float* dbeta_dev, int row_split, void* stream);

/* The small kernels between the GEMM stages of an update step, as single problems on the engine's own launchers (the launcher
 * picks the launch form, as it does inside a step).  Stand-alone for tests: every call builds its control record (batch slot 0,
 * metrics slot 0) and its scratch on the device and frees them before it returns.  All pointers are device memory.
 * `metrics_dev`: one record of 32 floats — [0..7] per-critic loss, [16] mean max_c |q_c - y|, [17] mean q, [18] actor loss,
 * [20] alpha loss, [21] alpha.
 *
 * gcrl_td_loss_f32: TD target, critic loss gradient and metrics.  r, d [B]; qt, q [C][B]; logp_next [B] (entropy targets) or
 * null; w [B] importance weights or null -> dq [C][B] = d loss_c / d q_c, td_abs [B] = max_c |q_c - y| (or null), metrics.
 *   target_kind 0: y = clamp(r + gamma (1 - d) qt_0, clamp_lo, 0)                         (src/agent.py:1317, C = 1)
 *               1: y = r + gamma (1 - d) min(qt_0, qt_1)                                   (src/agent.py:174-184, C = 2)
 *               2: ... min(qt_0, qt_1) - alpha logp_next                                   (src/agent.py:566-569, C = 2)
 *               3: ... mean of the C - drop lowest of the sorted qt_c - alpha logp_next    (src/agent.py:971-974)
 *   loss_kind   0: mse_loss, 1: smooth_l1_loss; with w: (w * loss(reduction="none")).mean() (src/agent.py:1320-1325)
 *   multi_block 0: the single-workgroup form.  n >= 1: the multi-workgroup form (taken at B >= 1024) with its partial-sum
 *               scratch and a zeroed ticket, launched n times into the same outputs; the ticket is zeroed once, and the
 *               outputs are filled with NaN patterns before every launch after the first, so what is read back is the
 *               last launch's work alone. */
int gcrl_td_loss_f32(const float* r_dev, const float* d_dev, const float* qt_dev, const float* q_dev, const float* logp_next_dev,
                     float alpha, const float* w_dev, int B, int C, int drop, int target_kind, int loss_kind, float gamma,
                     float clamp_lo, int multi_block, float* dq_dev, float* td_abs_dev, float* metrics_dev, void* stream);

/* SACActorModel.sample (src/model.py:118-141) on given head outputs: mu, ls_raw [B, ld_head] (first A columns), eps [B, A]
 * -> act [B, ld_act] (first A columns), logp [B], save_eps / save_std [B, A].  deterministic: act = tanh(mu) only (ls_raw,
 * eps, logp, save_eps, save_std may be null). */
int gcrl_tanh_gauss_fwd_f32(const float* mu_dev, const float* ls_raw_dev, int ld_head, const float* eps_dev, int B, int A,
                            int deterministic, float* act_dev, int ld_act, float* logp_dev, float* save_eps_dev,
                            float* save_std_dev, void* stream);
/* Its backward under the actor loss mean(alpha * logp - sel): dact [C][B][ld_dact] (the critics' action gradients, summed over
 * C), act [B, ld_act], eps / std [B, A] as the forward saved them, ls_raw [B, ld_head] -> gmu, gls [B, ld_g]: the gradients of
 * the two heads' outputs. */
int gcrl_tanh_gauss_bwd_f32(const float* dact_dev, int C, int ld_dact, const float* act_dev, int ld_act, const float* eps_dev,
                            const float* std_dev, const float* ls_raw_dev, int ld_head, float alpha, int B, int A,
                            float* gmu_dev, float* gls_dev, int ld_g, void* stream);

/* Actor-loss selection (src/agent.py:516-521: torch.min of two critics; :916-925: mean of the C - drop lowest of the sorted
 * ensemble) and the log-alpha loss / gradient (src/agent.py:532-546).  q [C][B], logp [B] -> dq [C][B] = d loss / d q_c,
 * metrics, grad_log_alpha (one float).  min_of_two (C = 2, drop = 0 only): SAC's torch.min; else the sorted form, which with
 * drop = 0 is the plain mean over the critics.  do_alpha = 0 stands for `gradient_step <= alpha_min_steps`.
 *   form 0: selection only (alpha as a literal; metrics[18]).
 *        1: selection + log-alpha gradient in one single-workgroup launch (alpha read from the device; metrics[18], [20],
 *           [21] when do_alpha = 0, and metrics[17] = mean(q) by the launch's rider workgroup).
 *        2: the same on the multi-workgroup form (taken at B >= 1024), launched twice as gcrl_td_loss_f32 does.
 *        3: form 2 launched once. */
int gcrl_actor_select_f32(const float* q_dev, const float* logp_dev, float alpha, int B, int C, int drop, int min_of_two,
                          int do_alpha, float target_entropy, float log_alpha, int form, float* dq_dev, float* metrics_dev,
                          float* grad_log_alpha_dev, void* stream);

/* The distributional TQC variant's loss kernels (gcrl_agent_config.n_quantiles > 1; no reference counterpart: the
 * specification is oracle/quantile_tqc_oracle.py).  r, d, logp_next [B]; zt, z [C][B][Q]: the target and online critics' atoms.
 * One wavefront sorts a row's C*Q pooled target atoms and keeps the lowest K = C*(Q - drop):
 *   y [B][64]: y_j = r + gamma (1 - d) (zt_(j) - alpha logp_next) for j < K, +0 for K <= j < 64 (all 64 words written)
 *   dz [C][B][Q] = d loss_c / d z_c, loss_c = mean over (B, Q, K) of |tau_i - 1(u < 0)| huber_1(u), u = y_j - z_c,i,
 *                  tau_i = (2i + 1) / (2Q)
 *   row_loss [C][B], row_td [B]: the per-row sums the metrics pass reduces; metrics[c] = loss_c for c < C,
 *                  metrics[16] = mean_b max_c |mean_j y_j - mean_i z_c,i|.
 * The launcher itself refuses C > 8, C*Q > 64 and drop outside [0, Q) (GCRL_ERR_ARG, "quantile_td: ..."), launching nothing. */
int gcrl_quantile_td_f32(const float* r_dev, const float* d_dev, const float* zt_dev, const float* z_dev,
                         const float* logp_next_dev, float alpha, int B, int C, int Q, int drop, float gamma, float* y_dev,
                         float* dz_dev, float* row_loss_dev, float* row_td_dev, float* metrics_dev, void* stream);
/* Its actor objective: loss = mean_b(alpha logp_b - mean over all C*Q atoms of z_c(s_b, pi(s_b))).  z [C][B][Q], logp [B]
 * -> dz [C][B][Q] = -1 / (B*C*Q) in every word, metrics[18] = loss. */
int gcrl_quantile_actor_f32(const float* z_dev, const float* logp_dev, float alpha, int B, int C, int Q, float* dz_dev,
                            float* metrics_dev, void* stream);

/* TD3 target-policy smoothing (src/agent.py:174-179), in place: act [B, ld] (first A columns) <- clamp(act +
 * clamp(eps * policy_noise, -noise_clip, noise_clip), -1, 1), eps [B, A]. */
int gcrl_td3_smooth_f32(float* act_dev, int ld, int B, int A, const float* eps_dev, float policy_noise, float noise_clip,
                        void* stream);

/* The device-RNG mode's Gaussian: out[i] = hash_normal(seed, ctr0 + i), the counter-hash Box-Muller normal that stands in
 * for torch.randn_like (src/agent.py:175, TD3 target smoothing) and Normal.rsample's eps (src/model.py:134) whenever an
 * update is not given injected noise.  Not torch's stream; restated in oracle/device_rng_oracle.py and tested against it. */
int gcrl_hash_normal_fill(uint64_t seed, uint64_t ctr0, int64_t n, float* out_dev, void* stream);

/* ---- Device-resident prioritised replay (csrc/per_tree.hip; DESIGN.md "Device-resident prioritised replay").
 * A tree of fp32 sums over one priority per PHYSICAL ring slot lives in HBM beside the ring: the proportional draw, the
 * importance-sampling weights and the priority update of the reference's PERBuffer (src/buffer.py:38-89) are HIP kernels on
 * it.  NOT the reference's index stream (np.random.choice): a device mode beside the host-drawn parity mode, defined by the
 * restatement tests/per_tree_ref.py.  A pushed row's slot gets priority 1.0; never-filled slots hold 0 and are never drawn.
 *
 * attach: build the (all-zero) tree for the ring's capacity; rows already in the ring count as pushed (priority 1.0).
 * alpha, eps: p = (|td| + eps)^alpha of the update. */
int gcrl_per_attach(gcrl_her* h, float alpha, float eps);
int gcrl_per_attached(const gcrl_her* h);
/* number of levels (leaves = level 0) and the padded entry count of one (a multiple of 64; -1: no such level) */
int gcrl_per_levels(const gcrl_her* h);
int64_t gcrl_per_level_size(const gcrl_her* h, int level);
/* In stream order: priority 1.0 for the rows pushed since the last draw (at most one launch), B proportional draws ->
 * idx_dev[B] (logical indices, what the gather reads), their weights (N p / total)^(-beta) / max -> w_dev[B] (may be null).
 * Advances the draw counter by one.  No host synchronisation.  GCRL_ERR_NOT_ENOUGH when the ring holds fewer than B rows. */
int gcrl_per_draw(gcrl_her* h, int B, float beta, uint32_t* idx_dev, float* w_dev, void* stream);
/* leaf of idx_dev[b] <- (|td_dev[b]| + eps)^alpha, the LAST occurrence of a duplicated index wins (src/buffer.py:86-89), the
 * touched ancestors recomputed; one launch, no host synchronisation. */
int gcrl_per_update(gcrl_her* h, const uint32_t* idx_dev, const float* td_dev, int B, void* stream);
/* The beta values of the update engine's next steps on this ring, one per step, consumed in order by the device-drawn path
 * of the agent update entries below (they travel as kernel arguments). */
int gcrl_per_set_betas(gcrl_her* h, const float* betas_host, int n);
/* priorities in logical order (0 = oldest row) on host arrays of exactly the ring's length; both synchronise.  set rebuilds
 * the whole tree (one launch per level), refuses negative / non-finite values and an all-zero array. */
int gcrl_per_get_priorities(gcrl_her* h, float* out_host, int64_t n);
int gcrl_per_set_priorities(gcrl_her* h, const float* in_host, int64_t n);
/* one level as stored (n = its padded size), pending pushes applied first; for tests and state */
int gcrl_per_read_level(gcrl_her* h, int level, float* out_host, int64_t n);
/* gcrl_her_sample's gather over n logical indices that are already on the device (each < capacity; what gcrl_per_draw wrote) */
int gcrl_her_sample_dev(gcrl_her* h, int64_t n, const uint32_t* idx_dev, float* out_s, int ld_s, float* out_a, int ld_a,
                        float* out_r, float* out_ns, int ld_ns, float* out_d, void* stream);
/* Move a FULL ring's rows so that logical row 0 lies at slot `head` (gcrl_her_load_state leaves it at 0).  The tree's sums depend
 * on where the leaves lie: a bitwise resume restores the saved head before gcrl_per_set_priorities.  Synchronises. */
int gcrl_her_set_head(gcrl_her* h, int64_t head);
/* the draw counter: number of the next draw (-1: no tree) */
int64_t gcrl_per_get_draw_counter(const gcrl_her* h);
int gcrl_per_set_draw_counter(gcrl_her* h, int64_t counter);
/* kernel launches the tree has issued so far (-1: no tree) */
int64_t gcrl_per_launches(const gcrl_her* h);

/* ---- Energy-prioritised replay draw of a GCRL_RELABEL_SAMPLE ring (csrc/her_prio.hip).
 * The ring gets a priority tree of the layout above whose leaves are written ONCE, by the flush: every row of a flushed episode
 * gets (E_traj + eps)^alpha / T, E_traj the clipped energy gains of the episode's achieved-goal trajectory (potential * ag[axis]
 * + kinetic * |ag_i - ag_{i-1}|^2 per step, one fp32 rounding per operation).  An episode is thereby drawn in proportion to its
 * energy and a row uniformly inside it.  Nothing feeds back from the loss, there are no importance-sampling weights: only the row
 * indices a gather reads change.  Definition: tests/her_energy_ref.py, held bit for bit (alpha == 1; otherwise 1e-6 relative).
 * The default constants (9.81, 312.5 = 0.5 / 0.04^2, axis 2, clip 0.5, alpha 1, eps 1e-3) are this project's choice.
 * gcrl_her_prio_attach: GCRL_RELABEL_SAMPLE rings only (GCRL_ERR_STATE otherwise), before or after rows exist — rows already in
 * the ring get the floor leaf eps^alpha (a zero-energy episode of one row, evaluated on the host) and the tree is rebuilt.
 * Refused: a ring that already has a tree of either kind (GCRL_ERR_STATE), axis >= goal_dim, clip <= 0, eps <= 0, alpha < 0,
 * a non-finite value, flush_len > 64 (GCRL_ERR_ARG).  gcrl_per_attach on such a ring stays refused; gcrl_per_draw / _update /
 * _set_betas refuse an energy tree; gcrl_per_get / set_priorities, gcrl_per_read_level and gcrl_per_launches serve both kinds.
 * With the tree attached, gcrl_her_sample and gcrl_her_gather_update called without indices draw their rows from it (the MT
 * stream is not consumed), and so does the update engine for every agent kind and launch form; gcrl_her_append is refused. */
typedef struct gcrl_energy_config {
  float potential;   /* m * g */
  float kinetic;     /* m / (2 dt^2) */
  int32_t axis;      /* component of the achieved goal that is a height; < 0: no potential term */
  float clip;        /* upper bound of one step's energy gain, > 0 */
  float alpha;       /* >= 0 */
  float eps;         /* > 0 */
} gcrl_energy_config;
enum { GCRL_PRIO_NONE = 0, GCRL_PRIO_ENERGY = 1, GCRL_PRIO_TD = 2 };
int gcrl_her_prio_attach(gcrl_her* h, const gcrl_energy_config* cfg);
int gcrl_her_prio_mode(const gcrl_her* h);
/* `rows` draws (with replacement) -> idx_dev[rows], logical indices; row t is the ring's (prio counter + t)-th draw and the
 * counter advances by `rows`: one call of n * B rows equals n calls of B.  One launch.  GCRL_ERR_STATE: no energy tree, or the
 * ring was reloaded and its leaves not yet set (gcrl_per_set_priorities). */
int gcrl_her_prio_draw(gcrl_her* h, int64_t rows, uint32_t* idx_dev, void* stream);
/* rows ever drawn from the ring's energy tree (0: no such tree); saved and restored by the caller for a bitwise resume */
uint64_t gcrl_her_get_prio_counter(const gcrl_her* h);
int gcrl_her_set_prio_counter(gcrl_her* h, uint64_t counter);

/* ---- TD-error prioritised replay of a GCRL_RELABEL_SAMPLE ring (csrc/her_td.hip; tests/her_td_ref.py is the
 * definition).  The ring gets a priority tree of the layout above, one leaf per stored transition, whose leaves follow the loss as
 * those of gcrl_per_attach do: a drawn row's leaf becomes (|td| + eps)^alpha (last occurrence of an index wins; alpha == 1: the
 * single fp32 add).  What differs is a NEW row's priority: one fp32 word p_max on the device, initially 1.0f, holds the largest
 * finite leaf value an update has produced; every row a flush launch writes gets the leaf p_max as that word stands in stream
 * order (one launch behind the flush, no host synchronisation), and rows present at attach time get its initial value.  p_max never
 * decreases; a NaN or infinite leaf value is written to its leaf and never raises it.
 * gcrl_her_td_attach: GCRL_RELABEL_SAMPLE rings only.  Refused, each naming `prioritise`: a GCRL_RELABEL_PUSH ring, a ring that has a
 * tree of any kind (GCRL_ERR_STATE), alpha not finite or < 0, eps not finite or not > 0 (GCRL_ERR_ARG).  gcrl_per_attach on such a
 * ring stays refused.  With the tree attached: gcrl_per_draw (draw + weights, N = the ring's length), gcrl_per_update (the update
 * above), gcrl_per_set_betas, gcrl_per_get / set_priorities, gcrl_per_read_level, gcrl_per_get / set_draw_counter and
 * gcrl_per_launches serve it; gcrl_her_prio_mode returns GCRL_PRIO_TD; gcrl_agent_update / gcrl_agent_update_n run the per-step loop
 * of a ring with a TD tree (draw, weights, the ring's own relabelling gather of those rows, the layer-per-launch step with the
 * weights, the update; scalar critics, pipeline_steps = 0, no gradient exchange, no prior ring, no behaviour-cloning term);
 * gcrl_pop_update_n and gcrl_pop_clone refuse such a ring, and so do gcrl_her_sample and gcrl_her_gather_update called without
 * indices (a uniform draw would pass for a prioritised one: draw with gcrl_per_draw, gather with gcrl_her_sample_dev) and
 * gcrl_her_append.  The TD error of whatever the gather produced for a drawn row, relabelled
 * or not, updates the stored row's one leaf.
 * gcrl_her_td_get_pmax (synchronises) / gcrl_her_td_set_pmax (finite, > 0): state and tests, never the loop. */
int gcrl_her_td_attach(gcrl_her* h, float alpha, float eps);
int gcrl_her_td_get_pmax(gcrl_her* h, float* out_host);
int gcrl_her_td_set_pmax(gcrl_her* h, float value);

/* ---- Prior-data replay: a fixed share of every batch from a second ring (csrc/her_prior.hip; DESIGN.md §4n;
 * tests/her_prior_ref.py is the definition).  An agent with a prior ring bound assembles every batch of B rows it gathers from its
 * own ring (gcrl_agent_update, gcrl_agent_update_n, gcrl_pop_update_n) so that
 *   - rows [0, B - rows) are bit for bit the rows the same call gathers without a prior ring: the main ring still draws B rows
 *     per batch, and its index stream, relabel counter and draw counter advance exactly as without one;
 *   - rows [B - rows, B) of batch j are batch j of the prior ring's own gather of `rows` rows per batch: bit for bit what
 *     gcrl_her_gather_update(prior, rows, n, NULL, ...) writes on a ring in the same state, with the agent's gamma as the discount
 *     of n-step windows.  The prior ring relabels, selects goals and normalises as IT is configured; its relabel counter advances
 *     by n * rows and its batch-draw counter by n, both snapshotted and advanced when the call is planned, after the main ring's.
 * The prior ring's existing gather writes the rows of a gather part into a scratch batch of the agent and ONE launch of
 * her_place_rows_kernel copies them over the tail rows of the batch slots: at most two extra launches per gather part, at most
 * four per call (a GCRL_NORMALIZE_SAMPLE prior ring adds its own normalise pass over the scratch to each part: three and six;
 * gcrl_agent_prior_counts counts the gathers and the placements).  Injected batches and caller-given row indices bypass the prior part.  The agent never pushes into the prior
 * ring; the caller fills it, between calls.  Without a prior ring nothing changes and no new kernel is launched.  This is the
 * symmetric sampling of RLPD and the replay half of "HER with demonstrations"; it is NOT the reference's sampling.
 * gcrl_agent_set_prior binds (prior != NULL, 1 <= rows <= batch_size - 1) or unbinds (NULL, 0); the ring is borrowed.  Refused,
 * naming prior_buffer or prior_rows — by gcrl_agent_set_prior (GCRL_ERR_ARG): rows outside 1..batch_size - 1; a ring whose rng
 * mode is not GCRL_RNG_DEVICE (its gather computes its own indices: no second index upload); a ring with a priority tree of
 * either kind; state or action widths other than the agent's — and by the update entries, before a ticket, an upload slot or a
 * row of any stream is consumed: fewer than `rows` rows in the prior ring (GCRL_ERR_NOT_ENOUGH); a goal width or a normalize mode
 * other than the main ring's, the main ring itself as its own prior, a main ring with a TD priority tree, an agent under a
 * gradient exchange (GCRL_ERR_STATE; the last is caution, not a measured limit). */
int gcrl_agent_set_prior(gcrl_agent* a, gcrl_her* prior, int rows);
int gcrl_agent_get_prior(const gcrl_agent* a, gcrl_her** prior_out, int* rows_out);
/* gathers of the prior ring and placement launches the agent has issued since creation (both 0 without a prior ring) */
int gcrl_agent_prior_counts(const gcrl_agent* a, int64_t* prior_gathers, int64_t* placements);
/* Batch slot `slot` (step `slot` of the last update call, 0 <= slot < min(gradient_step, 128)) as the call left it, to host arrays:
 * sa, nsa [batch_size][roundup(S + A, 4)], r, d [batch_size]; for tests and tools.  Synchronises the device.  The steps overwrite
 * nsa's columns from S on (the target policy's action); sa, nsa's state columns, r and d are the gathered batch. */
int gcrl_agent_read_batch(gcrl_agent* a, int slot, float* sa, float* nsa, float* r, float* d);
/* The same composition on two rings without an agent: gcrl_her_gather_update(main, B, M, NULL, outputs) followed by the prior ring's
 * gather of Bd rows per batch and the placement over rows [B - Bd, B) of each of the M batches (sa / nsa / spa [M * B][ldx], spa may
 * be NULL; r, d [M * B]).  Both rings' counters advance as by their own gathers.  The prior ring is held to the refusals above.
 * Allocates and frees its scratch and synchronises the stream: for tests and tools. */
int gcrl_her_gather_update_mixed(gcrl_her* main_ring, gcrl_her* prior, int B, int Bd, int M, float* sa, float* nsa, float* spa, int ldx,
                                 float* r, float* d, void* stream);

/* ---- Q-filtered behaviour cloning on the prior-data rows, DDPG and TD3 (csrc/her_bc.hip; tests/her_bc_ref.py is the
 * definition).  With the term on, an actor step on a batch of B rows whose last `rows` rows are demonstrations minimises
 *   L_actor = -mean_B Q0(s, pi(s)) + bc_weight * (1 / rows) * sum_{b >= B - rows} mask_b * sum_j (pi_bj - a_bj)^2
 * with Q0 the first critic as this step's critic update left it.  mask_b = 1 without the Q-filter; with it, mask_b = 1 where
 * Q0(s_b, a_b) > Q0(s_b, pi_b), strictly (a NaN on either side: 0).  The denominator is always `rows`.  The mask is a constant of the
 * step: no gradient flows through the comparison.  This is the loss of Nair et al. (ICRA 2018) in the form of OpenAI Baselines'
 * her/ddpg.py; it is NOT the reference's loss.
 * On the device: (q_filter) the stepped critic 0 runs a second forward over rows [B - rows, B) of [s | a] inside the launches of its
 * forward over [s | pi(s)] (no extra launch, hidden activations in scratch of its own), and ONE launch of bc_qfilter_kernel, between
 * the critic's input-gradient chain and the actor's backward, adds  (c * (pi - a)) * (1 - pi * pi), c = fp32(2 * bc_weight / rows), to
 * the accepted rows of the pre-tanh action gradient — rejected rows and rows below B - rows are not touched — and writes two words of
 * the step's metrics record: the term's value, bc_weight included, and the accepted share of the `rows` rows.  One extra launch per
 * actor step, none on critic-only TD3 steps, none at all without the term.  The update's result tuple does not change (its actor
 * loss stays -mean Q).  Named vectors "bc_q" and "bc_mask" [batch_size] (gcrl_agent_get): Q0(s, a) and the mask of the last actor
 * step, rows [B - rows, B); the other rows stay 0.  "bc_q_pi" [batch_size]: Q0(s, pi(s)) of that step; "batch_spa"
 * [min(gradient_step, 128)][batch_size][roundup(S + A, 4)]: the [s | pi(s)] rows of every batch slot as the actor steps left them.
 * gcrl_agent_set_bc: bc_weight > 0 and finite turns the term on for the last `rows` (1..batch_size) rows of every batch — the caller's
 * business that those rows are demonstrations (gcrl_agent_set_prior with the same count, or injected batches); bc_weight = 0 turns
 * it off.  Drops the captured step graphs.  Refused, naming bc_weight — by gcrl_agent_set_bc (GCRL_ERR_ARG): a weight that is
 * negative or not finite, rows outside 1..batch_size, SAC / TQC agents, agents on the row-chain or pipelined schedules
 * (pipeline_steps != 0) — and by the update entries, before a ticket, an upload slot or a row of any stream is consumed
 * (GCRL_ERR_STATE): an agent under a gradient exchange (gcrl_agent_set_exchange, gcrl_agent_dp_begin), steps with importance-sampling
 * weights (weights_host, a ring with a TD priority tree), population entries (gcrl_pop_update_n, gcrl_pop_clone). */
int gcrl_agent_set_bc(gcrl_agent* a, double bc_weight, int q_filter, int rows);
/* the settings in force (bc_weight 0: off) and the bc_qfilter_kernel launches issued or replayed since creation; any pointer may be NULL */
int gcrl_agent_get_bc(const gcrl_agent* a, double* bc_weight_out, int* q_filter_out, int* rows_out, int64_t* launches_out);
/* out2[0] = the behaviour-cloning term of the actor step with this (live) ticket, out2[1] = the accepted share of its demonstration
 * rows; waits for the ticket's call like gcrl_agent_metrics.  A ticket of a step without the term reads what its record slot held. */
int gcrl_agent_bc_metrics(gcrl_agent* a, int64_t ticket, double* out2);
/* The kernel alone, on raw device arrays, for tests: spa / sa [slots][B][ldx] with pi / the stored action in columns
 * [col0, col0 + A) of batch slot `slot`; q_pi [B]; q_a [B] or NULL (no filter); dact [B][ld_dact] updated in place; mask [B] (rows
 * [B - Bd, B) written) or NULL; metrics: one record of 32 floats, words [22] (term) and [23] (accepted share) written. */
int gcrl_bc_qfilter_f32(const float* spa_dev, const float* sa_dev, int ldx, int col0, int slots, int slot, const float* q_pi_dev,
                        const float* q_a_dev, int B, int Bd, int A, double bc_weight, float* dact_dev, int ld_dact, float* mask_dev,
                        float* metrics_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Device-resident goal environments, device-row acting entries and the collect loop.
 *
 * gcrl_env: N independent goal environments of one built-in kind in device memory — a one-member gcrl_env_group (below) under a
 * name and entries of its own (kernels csrc/dev_env.hip, host code csrc/dev_env_group.hip; the rule is restated in
 * tests/dev_env_ref.py, tests/dev_env_pick_ref.py and tests/dev_env_glide_ref.py, which are its definition).  G = 3, fixed horizon max_steps, sparse reward
 * -(dist > threshold) as the replay ring's built-in sparse kind forms it, no termination on success.  A is the kind's:
 * gcrl_env_dims reports it.  GCRL_ENV_REACH: A = 3, obs = [pos, vel, t/T] (7), achieved goal = pos.  GCRL_ENV_PUSH: A = 3, obs =
 * [pusher, puck, puck - pusher, pusher velocity, t/T] (13), achieved goal = puck.  GCRL_ENV_PICK: A = 4 (gripper velocity, finger
 * velocity), obs = [gripper, object, object - gripper, gripper velocity, object velocity, finger opening, finger velocity, held,
 * near, t/T] (20), achieved goal = object; the object is grasped when the fingers close around it, moves with the gripper while
 * they stay closed and falls when released; half the goals lie above the table.  GCRL_ENV_GLIDE: A = 3, obs = [pusher, puck, puck -
 * pusher, pusher velocity, puck velocity, t/T] (16), achieved goal = puck; a touched puck takes the pusher's displacement, a free one
 * keeps 0.9 of its last displacement per step, walls at x = -0.3 / 0.9 and y = +-0.3 stop that component; the goals lie at x in
 * [0.45, 0.65], beyond the pusher's box, so the puck has to be struck and let go.  Random numbers are a counter hash keyed by
 * (seed, episode index of the env, env, component): an env's episode j does not depend on N.
 * ---------------------------------------------------------------------------------------- */
typedef struct gcrl_env gcrl_env;
enum { GCRL_ENV_REACH = 0, GCRL_ENV_PUSH = 1, GCRL_ENV_PICK = 2, GCRL_ENV_GLIDE = 3 };
/* num_envs 1..1024, max_steps 1..64, 0 < threshold < 0.3 (push, pick, glide: 2 * threshold <= 0.15).  Every env starts at its episode 0. */
gcrl_env* gcrl_env_create(int kind, int num_envs, uint64_t seed, int max_steps, float threshold, int device);
void gcrl_env_destroy(gcrl_env* e);
int gcrl_env_dims(const gcrl_env* e, int* kind, int* num_envs, int* obs_dim, int* goal_dim, int* ac_dim, int* max_steps, float* threshold, uint64_t* seed);
/* Device addresses of the handle's blocks: rows [N][obs_dim + 3] = the acting rows [obs | goal] of the NEXT step; raw = the last
 * step's [obs N*D | next_obs N*D | dg N*3 | next_dg N*3 | ag N*3 | next_ag N*3]; pay [N][32] = t | reward | done = 0 | action(A) |
 * next_ag(3) — the layouts gcrl_agent_observe_act_dev and gcrl_her_process_step_dev read. */
int gcrl_env_buffers(gcrl_env* e, float** rows, float** raw, float** pay);
/* mask_host NULL: every env back to its episode 0, the counters to zero.  Else one byte per env: the selected envs go on to their
 * next episode (not counted as finished). */
int gcrl_env_reset(gcrl_env* e, const uint8_t* mask_host, void* stream);
/* One vector step, one launch: actions [N][A] on the device, float32 (actions_f64 == 0) or float64 (rounded to float32 first).  Any
 * action bits leave a finite state (a NaN component counts as 0).  An env that reaches the horizon is counted and re-seeded. */
int gcrl_env_step(gcrl_env* e, const void* actions_dev, int actions_f64, void* stream);
/* Synchronises.  Episodes finished, those that ended with dist < threshold, and the reward sum, over all envs since the last full reset. */
int gcrl_env_stats(gcrl_env* e, int64_t* episodes, int64_t* successes, double* reward_sum, void* stream);
/* State arrays (12 floats per env; pick: 18; glide: 15), counters, acting rows and the seed; resume is bitwise.  Loading refuses another kind, num_envs, max_steps or
 * threshold by that field's name before anything is overwritten. */
int64_t gcrl_env_state_bytes(const gcrl_env* e);
int gcrl_env_save_state(gcrl_env* e, void* dst_host, int64_t n, void* stream);
int gcrl_env_load_state(gcrl_env* e, const void* src_host, int64_t n, void* stream);
/* raw | pay of one vector step (the layout above, general dimensions) from separate contiguous float32 device tensors [n][.], one
 * launch.  ag_dev may be NULL (the ag and next_ag blocks of raw are then left alone; only a goal normaliser reads them).  The
 * payload's t word of env i is t_dev[i], or t0 when t_dev is NULL. */
int gcrl_proc_pack(const float* obs_dev, const float* next_obs_dev, const float* dg_dev, const float* next_dg_dev, const float* ag_dev,
                   const float* next_ag_dev, const float* actions_dev, const float* rewards_dev, const int32_t* t_dev, int t0, int n,
                   int obs_dim, int goal_dim, int action_dim, float* raw_out_dev, float* pay_out_dev, void* stream);
/* gcrl_agent_observe_act on DEVICE rows: rows_dev [n][state_dim] = raw [obs | goal] rows, noise_dev [n][A] float64 or NULL, float32
 * actions to out_f32_dev [n][A] — the float32 rounding of the float64 action the host entry returns, bit for bit.  It issues the
 * launch the host entry issues for staged rows (after the weight-copy rebuild where that entry does one), then one launch that rounds
 * the actions (and, for SAC / TQC with noise, one before it that rounds the eps, as the host entry stages it).  No copy, no
 * synchronisation.  n = 1..batch_size. */
int gcrl_agent_observe_act_dev(gcrl_agent* a, gcrl_normalizer* nz_obs, gcrl_normalizer* nz_dg, const float* rows_dev, int obs_dim, int n,
                               const double* noise_dev, int mode, float* out_f32_dev, void* stream);
/* gcrl_her_process_step_g on CALLER-OWNED device blocks in the layout above (on a normalize = "sample" ring: the raw-store form), with
 * the same host bookkeeping: staged counts, flushes, normaliser marks.  Nothing is uploaded, nothing is waited for.  dones_host NULL:
 * no env terminated (episodes end when flush_len rows are staged).  t_host[i]: the t word the caller wrote into env i's payload; it
 * must equal the ring's staged count of env0 + i, else GCRL_ERR_STATE naming `t` — checked on the host, before any launch.  A ring
 * with a host-callback reward is refused (compute_reward). */
int64_t gcrl_her_process_step_dev(gcrl_her* h, gcrl_normalizer* nz_obs, int update_stats, gcrl_normalizer* nz_dg, int update_goal_stats,
                                  const float* raw_dev, const float* pay_dev, int obs_dim, const int32_t* t_host, const uint8_t* dones_host,
                                  int env0, int n, void* stream);
/* The pick or glide kind's scripted controller (env_scripted_kernel, csrc/dev_env_script.hip; scripted_action of tests/dev_env_pick_ref.py
 * and of tests/dev_env_glide_ref.py is its definition), one launch: float32 actions [N][A] to out_dev (A = 4 / 3).  noise_std > 0 adds
 * float(double(hash_normal(seed, (counter * N + i) * A + j)) * noise_std) to element (i, j) before a final clamp to [-1, 1].  Refused: kind
 * (reach and push have no controller), noise_std (negative or not finite). */
int gcrl_env_scripted_act(gcrl_env* env, float* out_dev, double noise_std, uint64_t seed, uint64_t counter, void* stream);
/* `steps` vector steps of a pick or glide env under its scripted controller into ring, as a native loop: per step env_scripted_kernel, the env's
 * step on those float32 actions and the process-step launch on the env's blocks (gcrl_her_process_step_dev: its normaliser
 * arguments, its raw-store form on a normalize = "sample" ring), plus the flush launches — no host <-> device copy, no
 * synchronisation.  The noise of vector step s of the call is that of counter counter0 + s.  Fills any ring, a prior-data ring
 * included.  Refused by field name before anything is consumed, as gcrl_agent_collect refuses: env (more envs than ring slots;
 * dimensions; device), max_steps, compute_reward, threshold, steps, nz_obs / nz_dg, t, and kind (neither a pick nor a glide env), noise_std.
 * Returns the ring rows appended, or a negative error code. */
int64_t gcrl_her_collect_scripted(gcrl_her* ring, gcrl_env* env, gcrl_normalizer* nz_obs, gcrl_normalizer* nz_dg, int steps, double noise_std,
                                  uint64_t seed, uint64_t counter0, void* stream);
/* flush groups issued by the vector-step entries' bookkeeping since creation */
int64_t gcrl_her_flush_calls(const gcrl_her* h);
/* The exploration stream of gcrl_agent_collect: element (c, i, j) of vector step c is double(hash_normal(seed, (c N + i) A + j)) *
 * noise_std (SAC / TQC: the eps is that hash value); DDPG: with probability epsilon per vector step (one counter-hash uniform the
 * host evaluates) every env takes a clipped hash normal instead of the actor's action.  `counter` is c: part of a resume. */
int gcrl_agent_collect_set(gcrl_agent* a, uint64_t seed, double noise_std, double epsilon, uint64_t counter);
int gcrl_agent_collect_get(const gcrl_agent* a, uint64_t* seed, double* noise_std, double* epsilon, uint64_t* counter);
/* `steps` vector steps of env into ring as a native loop, in stream order per step: the acting launch on the env's rows, the env's
 * step, the process-step launch on the env's blocks, and the flush launches the ring's bookkeeping calls for — no host <-> device
 * copy and no synchronisation.  explore != 0: the stream above (mode 1 of gcrl_agent_observe_act); else its mode eval_mode.
 * Refused by field name before anything is consumed: env (more envs than ring slots, than batch_size or than 1024; dimensions that
 * differ from the agent's or the ring's; another device), max_steps (!= the ring's flush length), compute_reward (a ring whose reward
 * kind is not the built-in sparse one), threshold, steps (< 1), nz_obs / nz_dg (an update flag without its normaliser), t (the env
 * is not where the ring's staging area is).  *rows_out: ring rows appended. */
int gcrl_agent_collect(gcrl_agent* a, gcrl_env* env, gcrl_her* ring, gcrl_normalizer* nz_obs, int update_stats, gcrl_normalizer* nz_dg,
                       int update_goal_stats, int steps, int explore, int eval_mode, int64_t* rows_out, void* stream);
/* what gcrl_agent_collect and gcrl_agent_observe_act_dev have issued since creation; counted where issued (flush launches: declared
 * from the flush's definition — one per flush group, plus one per priority tree it seeds).  Any pointer may be NULL. */
int gcrl_agent_collect_counts(const gcrl_agent* a, int64_t* calls, int64_t* steps, int64_t* launches, int64_t* copies, int64_t* syncs);

/* ------------------------------------------------------------------------------------------
 * Environment groups, population collect and on-device evaluation.  Nothing here has a counterpart in the reference beyond its
 * trainer's test(path, num_episodes), which reports a success rate from a host loop.
 *
 * gcrl_env_group (csrc/dev_env_group.hip): members x num_envs envs in single allocations.  Member m IS a gcrl_env(kind, num_envs, seeds[m], ...): the same
 * state, counters, random-number keys and arithmetic (one step body, csrc/dev_env_body.h, shared by env_step_kernel and env_step_pop_kernel; the
 * definition stays tests/dev_env_ref.py, instantiated once per member).  The members' blocks are slices at the strides the
 * population kernels take: acting rows [members][stride_n][obs_dim + 3], step data [members][stride] floats with a member's slice
 * raw (raw_floats) | pay [num_envs][32], float64 noise / eps and float64 actions [members][stride_n][A].  stride_n > num_envs: the
 * rows past num_envs of a slice are never read and never written.  A group of one member launches env_step_kernel / env_reset_kernel
 * (the member's arguments by value, no table) where a group of several launches env_step_pop_kernel / env_reset_pop_kernel.
 * ---------------------------------------------------------------------------------------- */
typedef struct gcrl_env_group gcrl_env_group;
/* members 1..16, seeds[members]; the other arguments as gcrl_env_create.  Every env starts at its episode 0. */
gcrl_env_group* gcrl_env_group_create(int kind, int members, int num_envs, const uint64_t* seeds, int max_steps, float threshold, int device);
void gcrl_env_group_destroy(gcrl_env_group* g);
/* Any pointer may be NULL.  seeds_out[members]. */
int gcrl_env_group_dims(const gcrl_env_group* g, int* kind, int* members, int* num_envs, int* obs_dim, int* goal_dim, int* ac_dim, int* max_steps,
                        float* threshold, uint64_t* seeds_out, int* stride_n, int* stride, int* raw_floats);
/* Device addresses of the group's blocks in the layout above. */
int gcrl_env_group_buffers(gcrl_env_group* g, float** rows, float** data, double** noise64, double** act64);
/* One launch (env_reset_pop_kernel).  mask_host NULL: every env of every member back to its episode 0, the counters to zero.  Else
 * members x num_envs bytes: the selected envs go on to their next episode (not counted as finished). */
int gcrl_env_group_reset(gcrl_env_group* g, const uint8_t* mask_host, void* stream);
/* One vector step of every member, one launch (env_step_pop_kernel): actions_dev [members][num_envs][A], float32 or float64.
 * eps_members NULL, or one byte per member: a selected member's envs form their own actions,
 * clamp(hash_normal(eps_seeds[m], eps_ctr0[m] + env * A + component), -1, 1), and its slice of actions_dev is not read
 * (actions_dev may be NULL when every member is selected). */
int gcrl_env_group_step(gcrl_env_group* g, const void* actions_dev, int actions_f64, const uint8_t* eps_members, const uint64_t* eps_seeds,
                        const uint64_t* eps_ctr0, void* stream);
/* Synchronises once.  Per member, what gcrl_env_stats reports for it: episodes[members], successes[members], reward_sum[members]. */
int gcrl_env_group_stats(gcrl_env_group* g, int64_t* episodes, int64_t* successes, double* reward_sum, void* stream);
/* The blob is a 24-byte group header followed by one record per member, each byte for byte what gcrl_env_save_state writes for a
 * standalone env in that member's state; resume is bitwise.  Loading refuses other members, kind, num_envs, max_steps or threshold
 * by that field's name before anything is overwritten. */
int64_t gcrl_env_group_state_bytes(const gcrl_env_group* g);
int gcrl_env_group_save_state(gcrl_env_group* g, void* dst_host, int64_t n, void* stream);
int gcrl_env_group_load_state(gcrl_env_group* g, const void* src_host, int64_t n, void* stream);
/* Deterministic evaluation: ceil(episodes / N) * max_steps vector steps of the acting launch in mode eval_mode (gcrl_agent_observe_act's
 * mode 0 or 2 for DDPG / TD3, 2 for SAC / TQC: tanh(mean)) followed by the env's step — two launches a step, no ring, no process-step;
 * the normalisers are read and never updated and the exploration stream does not move.  reset != 0: gcrl_env_reset(env, NULL) first,
 * so the call scores episodes 0, 1, ... of the env's seed.  reset == 0: every env must stand at step 0 of an episode (else
 * GCRL_ERR_STATE naming `t`); the result is the counters' difference over the call.  One synchronisation, at the end.  *episodes_out
 * (a multiple of N: what was run), *successes_out, *reward_sum_out.  Refused by field name before anything is launched: env
 * (more envs than batch_size, other dimensions, another device), episodes (< 1), nz_obs / nz_dg (sizes), t. */
int gcrl_agent_evaluate(gcrl_agent* a, gcrl_env* env, gcrl_normalizer* nz_obs, gcrl_normalizer* nz_dg, int episodes, int reset, int eval_mode,
                        int64_t* episodes_out, int64_t* successes_out, double* reward_sum_out, void* stream);
/* gcrl_agent_collect for all members of a population on a group, as a native loop; per vector step, in stream order, ONE launch each
 * for all members: (a) the population acting launch on the group's rows (after each member's last update call and its weight-copy
 * rebuild where due; a DDPG member on its epsilon branch is not in it, and with every member there the launch is not issued),
 * (b) env_step_pop_kernel, which reads the float64 actions, forms an epsilon member's actions itself and leaves each member's noise of
 * its NEXT vector step, (c) the population process-step launch on the group's blocks, followed by the rings' flush launches in member
 * order.  No host <-> device copy and no synchronisation.  Each member keeps its own exploration stream (gcrl_agent_collect_set; element
 * (c, i, j) with N = envs per member) and its counter; a first call, or a re-keyed stream, pays one fill launch per member concerned.
 * Member m then holds, bit for bit, what a standalone agent's gcrl_agent_collect on gcrl_env(seeds[m]) leaves.  A one-member
 * population runs the member's own gcrl_agent_collect loop on the group.  rows_out[members]: ring rows appended per member.
 * Refused by field name before anything is consumed: env (null; members != the population's; more envs per member than ring slots,
 * batch_size or 1024; dimensions; device), max_steps, threshold, compute_reward, steps, nz_obs / nz_dg, normalize, t (naming the
 * member and the env), shared_ring (two members with one ring). */
int gcrl_pop_collect(gcrl_pop* p, gcrl_env_group* g, gcrl_her* const* rings, gcrl_normalizer* const* nz_obs, int32_t update_stats,
                     gcrl_normalizer* const* nz_dg, int32_t update_goal_stats, int32_t steps, int32_t explore, int32_t eval_mode, int64_t* rows_out,
                     void* stream);
/* what gcrl_pop_collect has issued since creation, counted as gcrl_agent_collect_counts counts.  Any pointer may be NULL. */
int gcrl_pop_collect_counts(const gcrl_pop* p, int64_t* calls, int64_t* steps, int64_t* launches, int64_t* copies, int64_t* syncs);
/* gcrl_agent_evaluate for all members on a group: the population acting launch in eval mode and env_step_pop_kernel, two launches a
 * step for all members, one synchronisation at the end; episodes_out / successes_out / reward_sum_out [members].  reset != 0 resets
 * the whole group first.  Refusals as gcrl_agent_evaluate's, `env` also for a group of another member count. */
int gcrl_pop_evaluate(gcrl_pop* p, gcrl_env_group* g, gcrl_normalizer* const* nz_obs, gcrl_normalizer* const* nz_dg, int32_t episodes, int32_t reset,
                      int32_t eval_mode, int64_t* episodes_out, int64_t* successes_out, double* reward_sum_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Practice goals (csrc/goal_propose.hip; tests/goal_propose_ref.py is the definition).  Nothing here has a counterpart in the
 * reference.  A proposer owns an archive, a circular buffer of `capacity` raw achieved goals [capacity][3] float32 in the env's own
 * units, and serves ONE gcrl_env of N envs, bound at its first use.  Behind every vector step of that env, in stream order:
 *   append   the step's N next_ag rows go to logical positions len .. len + N - 1; a full archive drops its oldest entries;
 *   propose  only in a step in which an env rolled over (its host t was max_steps - 1 before the step; an env put to t = 0 by
 *            gcrl_env_reset has not rolled over and keeps its task goal): the counter q is read, then incremented; with L = len >=
 *            min_fill every rolled-over env i takes a proposal iff float(hash_below(seed, TAKE, q N + i, 2^24)) * 2^-24 < share; its
 *            candidate k = 0 .. C - 1 is logical index hash_below(seed, CAND, (q N + i) C + k, L); a candidate's count is the number
 *            of archive entries m in [0, L) with ((dx dx + dy dy) + dz dz) < radius * radius in float32 without contraction (it
 *            counts itself); the smallest count wins, ties to the smallest k; the winner's three words go to floats 9..11 of the
 *            env's state record and to columns obs_dim .. obs_dim + 2 of its acting row.  The finished step's raw / pay blocks keep
 *            the old goal.  TAKE = 0x5052414354414b45, CAND = 0x5052414343414e44; hash_below is the replay ring's counter hash.
 * The env's stats count an episode's success against the goal the episode had, practised or task; gcrl_agent_evaluate never
 * appends and never proposes, and with reset != 0 scores task goals only.
 * ---------------------------------------------------------------------------------------- */
typedef struct gcrl_goal_proposer gcrl_goal_proposer;
/* Refused naming the field, in this order: capacity (1..65536), candidates (1..64), radius (finite, > 0), share (in (0, 1]),
 * min_fill (1..capacity); then a device that is not usable.  NULL on failure. */
gcrl_goal_proposer* gcrl_goal_proposer_create(int capacity, int candidates, float radius, float share, int min_fill, uint64_t seed, int device);
void gcrl_goal_proposer_destroy(gcrl_goal_proposer* p);
/* The binding rules on plain numbers, as gcrl_goal_proposer_step and gcrl_agent_collect_practice apply them to their handles (no
 * device needed): members (env_members != 1), device (env_device != device), env (bound_num_envs != 0 and another env handle or
 * another env count), capacity (< env_num_envs). */
int gcrl_goal_proposer_bind_check(int capacity, int bound_num_envs, int same_env, int device, int env_members, int env_num_envs, int env_device);
/* The host-loop entry, called after gcrl_env_step on the same stream: goal_archive_append_kernel and, as above, goal_propose_kernel
 * (one workgroup per rolled-over env); one or two launches, no copy, no synchronisation.  Refused before anything is consumed:
 * the binding rules above, and with GCRL_ERR_STATE naming `env` when the env has not stepped since the proposer's last step. */
int gcrl_goal_proposer_step(gcrl_goal_proposer* p, gcrl_env* env, void* stream);
/* rows appended, steps in which an env rolled over, proposals patched — since creation (or as loaded).  Any pointer may be NULL. */
int gcrl_goal_proposer_stats(const gcrl_goal_proposer* p, int64_t* appended, int64_t* roll_steps, int64_t* patched);
/* Settings, the bound env count (0: not bound), head (slot of the oldest entry), len, the counter q, and the number of archive slots
 * goal_propose_kernel stages per pass.  Any pointer may be NULL. */
int gcrl_goal_proposer_get(const gcrl_goal_proposer* p, int* capacity, int* candidates, float* radius, float* share, int* min_fill, uint64_t* seed,
                           int* device, int* num_envs, int* head, int* len, uint64_t* counter, int* tile);
/* The archive in logical order, len * 3 floats, to host memory.  Synchronises. */
int gcrl_goal_proposer_read(gcrl_goal_proposer* p, float* dst_host, void* stream);
/* An 80-byte header (magic, capacity, candidates, min_fill, radius, share, seed, num_envs, head, len, pad, q, the three stats) and the
 * archive's capacity * 3 floats at their physical slots; resume is bitwise.  Loading refuses other settings (capacity, candidates,
 * radius, share, min_fill, seed), another num_envs than the handle is bound to, and a head or len outside the archive, by that
 * field's name before anything is overwritten.  Save behind gcrl_goal_proposer_step, not between it and the env's step. */
int64_t gcrl_goal_proposer_state_bytes(const gcrl_goal_proposer* p);
int gcrl_goal_proposer_save_state(gcrl_goal_proposer* p, void* dst_host, int64_t n, void* stream);
int gcrl_goal_proposer_load_state(gcrl_goal_proposer* p, const void* src_host, int64_t n, void* stream);
/* gcrl_agent_collect with the proposer's launches behind each env step: the same loop, arguments and refusals, plus the proposer's
 * (members, device, env, capacity), all before anything is consumed.  No copy, no synchronisation;
 * gcrl_agent_collect_counts' launches grow by one more per step (the append) and one more per step in which an env rolled over and
 * the archive held min_fill entries (the propose). */
int gcrl_agent_collect_practice(gcrl_agent* a, gcrl_env* env, gcrl_her* ring, gcrl_normalizer* nz_obs, int update_stats, gcrl_normalizer* nz_dg,
                                int update_goal_stats, int steps, int explore, int eval_mode, gcrl_goal_proposer* proposer, int64_t* rows_out, void* stream);

/* hipEvent helpers so a Python caller can time the engine's own stream (torch.cuda.Event only
 * sees torch's current stream). */
void* gcrl_event_create(void);
void gcrl_event_destroy(void* ev);
int gcrl_event_record(void* ev, void* stream);
int gcrl_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms_out); /* syncs on stop */
int gcrl_stream_synchronize(void* stream);
/* plain device memory for callers without torch */
void* gcrl_malloc(size_t bytes);
void gcrl_free(void* p);
int gcrl_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes, void* stream);
int gcrl_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GCRL_H */
