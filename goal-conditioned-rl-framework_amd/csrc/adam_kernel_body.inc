// adam_kernel_body.inc — body of the optimiser launch, included by ops.hip into adam_kernel (the single-agent launch) and by
// adam_pop.hip into adam_pop_kernel (the population launch).  In scope: `a` (the launch's AdamArgs).
  // round 5: the metric riders (TD metrics of 2 048 rows x 2 critics at TD3's cfg 3: one memory round trip and four block reductions) have a
  // workgroup of their own — the launch's last — instead of extending workgroup 0's norm -> step chain
  const bool extra = a.mean_x || a.td_q;
  if (extra && blockIdx.x == gridDim.x - 1) {
    if (blockIdx.y == 0) adam_riders(a, *a.cur);
    return;
  }
  adam_body(a, blockIdx.y, false, gridDim.x - (extra ? 1u : 0u));
  if (a.alpha.log_alpha && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) alpha_step(a.alpha, *a.cur);
  advance_ctrl(a);
