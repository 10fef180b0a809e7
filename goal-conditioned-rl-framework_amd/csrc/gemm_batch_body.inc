// gemm_batch_body.inc — body of the batched GEMM launch, included by gemm_mfma.h into gemm_batch_kernel (the single-agent launch)
// and gemm_batch_pop_kernel (the population launch).  In scope: template <int TM, int TN, int KSPLIT>, `gb` (the launch's GemmBatch).
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bid = xcd_tile_of((int)blockIdx.x, (int)gridDim.x);
  const int wtile = (KSPLIT == 4) ? bid : bid * 4 + wave;
  const int pi = gemm_problem_of(gb, wtile);
  const GemmDesc& d = gb.d[pi];
  gemm_pin(d);
  const int t = wtile - d.tile0;
  float x, ss;
  if (!gemm_batch_tile<TM, TN, KSPLIT>(d, t, x, ss)) return;
  if (d.sumsq_out) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_down(ss, off, 64);
    if (lane == 0) d.sumsq_out[(long long)t * KSPLIT + (KSPLIT == 4 ? wave : 0)] = ss;
  }
