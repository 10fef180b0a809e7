// her_gather_update_body.inc — the body of her_gather_update_kernel<kHead, kNT> and of its population form
// her_gather_update_pop_kernel<kHead> (her_ring.hip), included into both: `p` is the launch's GatherUpdArgs (the kernel argument;
// in the population form the member's entry copied into a local struct), kHead / kNT the including kernel's template parameters.
// One text, so a member's rows are the bits its own launch writes, and the single-agent kernel keeps its ISA.
  extern __shared__ float gather_lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sub = lane >> 4, v4 = lane & 15;
  if (kHead)
    for (int i = blockIdx.x * 256 + threadIdx.x; i < p.cp_n16; i += gridDim.x * 256) p.cp_dst[i] = p.cp_src[i];
  const int SA4 = p.SA4, S4 = p.S4, o_r = SA4 + S4;
  const int nq = 4 * SA4;                                   // 16-byte quads of a [16][SA4] tile
  float* tile = gather_lds + (size_t)w * (8 * nq + 32);     // [sa 16 x SA4 | nsa 16 x SA4 | r 16 | d 16]
  float* t_ns = tile + 4 * nq;
  float* t_rd = tile + 8 * nq;
  const long long r0 = ((long long)blockIdx.x * 4 + w) * 16;
  if (r0 >= p.n) return;
  uint32_t ph32 = 0;
  if (lane < 16 && r0 + lane < p.n) {
    unsigned long long phys = (unsigned long long)p.head + (p.idx ? p.idx[r0 + lane] : gcrl::idxgen_at(p.gen, r0 + lane));
    if (phys >= (unsigned long long)p.cap) phys -= (unsigned long long)p.cap;    // head, index < cap
    ph32 = (uint32_t)phys;
  }
  const bool full = r0 + 16 <= p.n;
  // records wider than 64 floats (state dims above ~28) take further 64-float column passes
  for (int cc = 0; cc <= o_r; cc += 64) {
    const int c0 = cc + v4 * 4;
    const bool useful = c0 <= o_r;
    float4 val[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t ph = __shfl(ph32, u * 4 + sub, 64);
      val[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (useful && r0 + u * 4 + sub < p.n) val[u] = *reinterpret_cast<const float4*>(p.ring + (size_t)ph * p.RS + c0);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int rl = u * 4 + sub;
      const long long row = r0 + rl;
      if (!useful || row >= p.n) continue;
      if (p.spa && c0 < S4) *reinterpret_cast<float4*>(p.spa + row * p.ldx + c0) = val[u];   // layer-per-launch schedules only
      if (full) {
        if (c0 < SA4) *reinterpret_cast<float4*>(tile + rl * SA4 + c0) = val[u];
        else if (c0 < o_r) *reinterpret_cast<float4*>(t_ns + rl * SA4 + (c0 - SA4)) = val[u];
        else { t_rd[rl] = val[u].x; t_rd[16 + rl] = val[u].y; }
      } else {   // the launch's last, partial wave: straight from the load lanes
        if (c0 < SA4) *reinterpret_cast<float4*>(p.sa + row * p.ldx + c0) = val[u];
        else if (c0 < o_r) *reinterpret_cast<float4*>(p.nsa + row * p.ldx + (c0 - SA4)) = val[u];
        else { p.r[row] = val[u].x; p.d[row] = val[u].y; }
      }
    }
  }
  if (!full) return;
  const int zq = (SA4 - S4) >> 2;          // quads of an nsa row beyond the record's ns group (<= 5: action_dim <= 16)
  if (v4 < zq) {
#pragma unroll
    for (int u = 0; u < 4; ++u) *reinterpret_cast<float4*>(t_ns + (u * 4 + sub) * SA4 + S4 + v4 * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // the tile is private to this wave and a wave's LDS operations execute in order: no barrier, only the compiler is held back
  __builtin_amdgcn_wave_barrier();
  float* sa = p.sa + r0 * p.ldx;
  float* nsa = p.nsa + r0 * p.ldx;
  const bool rd_vec = ((reinterpret_cast<size_t>(p.r) | reinterpret_cast<size_t>(p.d)) & 15) == 0;
  const int Q = 2 * nq + (rd_vec ? 8 : 0);
  for (int q = lane; q < Q; q += 64) {
    const float4 v = *reinterpret_cast<const float4*>(tile + q * 4);
    float* dst = q < nq ? sa + q * 4 : q < 2 * nq ? nsa + (q - nq) * 4 : q < 2 * nq + 4 ? p.r + r0 + (q - 2 * nq) * 4 : p.d + r0 + (q - 2 * nq - 4) * 4;
    if (kNT) store4_nt(dst, v);
    else *reinterpret_cast<float4*>(dst) = v;
  }
  if (!rd_vec && lane < 32) (lane < 16 ? p.r : p.d)[r0 + (lane & 15)] = t_rd[lane];
