// pbt_host_check.cc — the host code of the population's clone / re-tune / replace entries (csrc/pbt_host.h: argument checks, the segment
// table of pop_clone_kernel, the schedule replay) as a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -DGCRL_HOST_ONLY
//       tools/pbt_host_check.cc goal-conditioned-rl-framework_amd/csrc/lr_sched.cc -o pbt_host_check && ./pbt_host_check
// (make -C goal-conditioned-rl-framework_amd/csrc pbt_asan does both).  CPU only; prints "pbt host check: ok" and exits 0.
#include <cstdlib>
#include <cstring>
#include <string>

#include "../goal-conditioned-rl-framework_amd/csrc/pbt_host.h"

using namespace gcrl;

static int fails = 0;
#define EXPECT(cond)                                                             \
  do {                                                                           \
    if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } \
  } while (0)

static bool refused(int members, std::vector<int32_t> s, std::vector<int32_t> d, int pairs, uint32_t what, const char* field) {
  char why[96];   // (shorter than any caller's buffer: truncation must stay inside it)
  std::memset(why, 0x7f, sizeof(why));
  const bool ok = pop_clone_check(members, s.empty() ? nullptr : s.data(), d.empty() ? nullptr : d.data(), pairs, what, why, sizeof(why));
  return !ok && std::strstr(why, field) == why;
}

int main() {
  char why[256];
  // ---- gcrl_pop_clone's arguments
  EXPECT(pop_clone_check(3, std::vector<int32_t>{0}.data(), std::vector<int32_t>{2}.data(), 1, GCRL_CLONE_AGENT, why, sizeof(why)));
  EXPECT(pop_clone_check(3, std::vector<int32_t>{0, 0}.data(), std::vector<int32_t>{1, 2}.data(), 2, GCRL_CLONE_AGENT | GCRL_CLONE_RING, why, sizeof(why)));
  EXPECT(refused(3, {}, {1}, 1, 1, "src:"));
  EXPECT(refused(3, {0}, {}, 1, 1, "dst:"));
  EXPECT(refused(3, {0}, {1}, 0, 1, "pairs:"));
  EXPECT(refused(3, {0}, {1}, 17, 1, "pairs:"));
  EXPECT(refused(3, {0}, {1}, -5, 1, "pairs:"));
  EXPECT(refused(3, {0}, {1}, 1, 0, "what:"));
  EXPECT(refused(3, {0}, {1}, 1, 4, "what:"));
  EXPECT(refused(3, {3}, {1}, 1, 1, "src:"));
  EXPECT(refused(3, {0}, {-1}, 1, 1, "dst:"));
  EXPECT(refused(3, {0, 1}, {1, 2}, 2, 1, "dst: member 1 is both"));
  EXPECT(refused(3, {0, 1}, {2, 2}, 2, 1, "dst: member 2 is a destination twice"));
  {   // 16 members, 16 pairs is over any population's reach without an overlap: 8 sources, 8 destinations pass
    std::vector<int32_t> s, d;
    for (int k = 0; k < 8; ++k) { s.push_back(k); d.push_back(8 + k); }
    EXPECT(pop_clone_check(16, s.data(), d.data(), 8, 1, why, sizeof(why)));
    s.assign(16, 15);
    d.clear();
    for (int k = 0; k < 16; ++k) d.push_back(k);
    EXPECT(!pop_clone_check(16, s.data(), d.data(), 16, 1, why, sizeof(why)) && std::strstr(why, "member 15 is both"));
  }
  // ---- the segment table
  {
    std::vector<float> src(10 * 16), dst(10 * 16);
    std::vector<CloneSeg> t;
    clone_add(t, src.data(), dst.data(), 0);
    EXPECT(t.empty());
    // capacity 10, head 7, len 10 (wrapped): rows 7..9 then 0..6, into the destination from row 0
    clone_add_ring_rows(t, src.data(), dst.data(), 7, 10, 10, 16);
    EXPECT(t.size() == 2);
    EXPECT(t[0].src == src.data() + 7 * 16 && t[0].dst == dst.data() && t[0].bytes == 3 * 16 * sizeof(float));
    EXPECT(t[1].src == src.data() && t[1].dst == dst.data() + 3 * 16 && t[1].bytes == 7 * 16 * sizeof(float));
    unsigned long long total = 0;
    for (const CloneSeg& s : t) {
      EXPECT((const char*)s.src >= (const char*)src.data() && (const char*)s.src + s.bytes <= (const char*)(src.data() + src.size()));
      EXPECT((char*)s.dst >= (char*)dst.data() && (char*)s.dst + s.bytes <= (char*)(dst.data() + dst.size()));
      std::memcpy(s.dst, s.src, s.bytes);   // (what the kernel does: the sanitizer sees every byte of every segment)
      total += s.bytes;
    }
    EXPECT(total == 10 * 16 * sizeof(float));
    t.clear();
    clone_add_ring_rows(t, src.data(), dst.data(), 0, 4, 10, 16);   // not yet wrapped: one piece, only the filled part
    EXPECT(t.size() == 1 && t[0].bytes == 4 * 16 * sizeof(float));
    t.clear();
    clone_add_ring_rows(t, src.data(), dst.data(), 0, 0, 10, 16);   // empty ring: nothing
    EXPECT(t.empty());
    EXPECT(clone_chunks(t, 128) == 1);
    t.push_back(CloneSeg{src.data(), dst.data(), 16384 * 3 + 1});
    EXPECT(clone_chunks(t, 128) == 4 && clone_chunks(t, 2) == 2);
    t.push_back(CloneSeg{src.data(), dst.data(), 1ull << 40});
    EXPECT(clone_chunks(t, 128) == 128);
  }
  // ---- gcrl_agent_set_hparams' values
  {
    gcrl_hparams h{1e-3, 1e-4, 1e-3, 1e-4, 10, 10, 0.98, 0.05, 1.0, 3e-4, 100.0};
    EXPECT(hparams_check(&h, true, why, sizeof(why)));
    EXPECT(!hparams_check(nullptr, true, why, sizeof(why)) && std::strstr(why, "h:") == why);
    auto bad = [&](gcrl_hparams x, bool sac, const char* field) {
      char w[64];
      return !hparams_check(&x, sac, w, sizeof(w)) && std::strstr(w, field) == w;
    };
    gcrl_hparams x = h; x.actor_lr = 0.0; EXPECT(bad(x, false, "actor_lr:"));
    x = h; x.critic_lr = -1.0; EXPECT(bad(x, false, "critic_lr:"));
    x = h; x.actor_lr_min = -1e-9; EXPECT(bad(x, false, "actor_lr_min:"));
    x = h; x.critic_lr = std::nan(""); EXPECT(bad(x, false, "critic_lr:"));
    x = h; x.ac_scheduler_steps = 0; EXPECT(bad(x, false, "ac_scheduler_steps:"));
    x = h; x.cr_scheduler_steps = -3; EXPECT(bad(x, false, "cr_scheduler_steps:"));
    x = h; x.gamma = std::nan(""); EXPECT(bad(x, false, "gamma:"));
    x = h; x.tau = std::nan(""); EXPECT(bad(x, false, "tau:"));
    x = h; x.grad_clip = std::nan(""); EXPECT(bad(x, false, "grad_clip:"));
    x = h; x.grad_clip = -1.0; x.gamma = 1.0; x.tau = 0.0; EXPECT(hparams_check(&x, false, why, sizeof(why)));   // (as a constructor takes them)
    {
      gcrl_agent_config c;
      std::memset(&c, 0, sizeof(c));
      c.actor_lr = 1e-3; c.critic_lr = 2e-3; c.ac_scheduler_steps = 3; c.cr_scheduler_steps = 4; c.gamma = 0.9; c.tau = 0.1; c.grad_clip = -1.0;
      gcrl_hparams y = hparams_of(c);
      EXPECT(y.actor_lr == 1e-3 && y.critic_lr == 2e-3 && y.ac_scheduler_steps == 3 && y.cr_scheduler_steps == 4 && y.gamma == 0.9 && y.tau == 0.1);
      EXPECT(hparams_check(&y, false, why, sizeof(why)));
      c.critic_lr = 0.0; y = hparams_of(c); EXPECT(bad(y, false, "critic_lr:"));
    }
    x = h; x.alpha_lr = 0.0; EXPECT(bad(x, true, "alpha_lr:")); EXPECT(hparams_check(&x, false, why, sizeof(why)));
  }
  // ---- the schedule replayed at a kept position is the recursion itself
  {
    double lr = 1e-3;
    for (int64_t e = 1; e <= 37; ++e) lr = gcrl_cosine_lr_next(lr, 1e-3, 1e-4, 30, e);
    EXPECT(cosine_lr_at(1e-3, 1e-4, 30, 37) == lr);
    EXPECT(cosine_lr_at(1e-3, 1e-4, 30, 0) == 1e-3);
  }
  // ---- the shared fields of a replacement
  {
    gcrl_agent_config a;
    std::memset(&a, 0, sizeof(a));
    a.hidden_dim = 64; a.batch_size = 64; a.layer_count = 2; a.ac_update_freq = 2; a.num_critics = 2;
    gcrl_agent_config b = a;
    b.gamma = 0.5; b.seed = 9; b.actor_lr = 1.0;
    EXPECT(pop_mismatch(a, b) == nullptr);
    b = a; b.hidden_dim = 128; EXPECT(std::string(pop_mismatch(a, b)) == "hidden_dim");
    b = a; b.batch_size = 32; EXPECT(std::string(pop_mismatch(a, b)) == "batch_size");
    b = a; b.layer_count = 3; EXPECT(std::string(pop_mismatch(a, b)) == "layer_count");
    b = a; b.ac_update_freq = 1; EXPECT(std::string(pop_mismatch(a, b)) == "ac_update_freq");
    b = a; b.num_critics = 5; EXPECT(std::string(pop_mismatch(a, b)) == "num_critics");
  }
  std::printf(fails ? "pbt host check: %d FAILED\n" : "pbt host check: ok\n", fails);
  return fails ? 1 : 0;
}
