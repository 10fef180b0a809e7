// adam_pair_body.inc — body of the paired optimiser launch, included by ops.hip into adam_pair_kernel (the single-agent launch) and
// by adam_pop.hip into adam_pair_pop_kernel (the population launch).  In scope: `a0`, `a1` (the launch's two AdamArgs).
  if (blockIdx.y == 0) adam_body(a0, 0);
  else adam_body(a1, 0);
  advance_ctrl(a0);
