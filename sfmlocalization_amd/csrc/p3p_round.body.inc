// the body of k_p3p_round (acransac.hip): included by the kernel itself and by its gang form's Body::run, so that
// the kernel compiles exactly as if the text stood in it (an inlined call does not: the loops are unrolled and scheduled
// before the inlining, and the scan lost 20 % that way)
  P3pState &st = *A.state;
  if (st.done) return;
  // (kForm: a constant of the including function -- 0 the full form, 1 the small form k_p3p_round_small; kSolver: 0 P3P,
  // 1 the six-point resection of an uncalibrated query)
  // a small round on a set it is not built for: not this launch's business (every workgroup leaves, nothing is counted or
  // written; the host queues the query's rounds again in the full form)
  if (kForm == 1 && st.n > kP3pSmallN) return;
  // a WIDE launch has four workgroups per hypothesis, one per model ("single" mode: the workgroup's four waves share the
  // model's residuals, sort and NFA scan) -- the form of a query alone on the GPU and of large match sets.  Beyond the LDS
  // forms (more than kP3pMaxN correspondences) only workgroup b works -- the others leave here, uncounted -- and the round
  // is what it is in a plain launch.
  const int single_mode = (wide && st.n <= kP3pMaxN) ? 1 : 0;
  // (model m of hypothesis b is workgroup m * (gridDim.x / 4) + b: the workgroups that always work have the lowest
  // indices and are dispatched first -- the ones that leave here never hold a compute unit's LDS in front of them)
  if (wide && !single_mode && blockIdx.x >= gridDim.x / 4u) return;
  const unsigned expected_arrivals = (wide && !single_mode) ? gridDim.x / 4u : gridDim.x;
  extern __shared__ unsigned char smem_raw[];
  {
    const int per_model = wide ? (int)(gridDim.x >> 2) : (int)gridDim.x;  // hypotheses of the launch
    p3p_eval_hypothesis<kForm, kSolver>(A, batch, wide, smem_raw, (int)blockIdx.x % per_model, (int)blockIdx.x / per_model);
  }
  __shared__ unsigned s_ticket;
  // producer rule (MI355X_MICROARCH.md, hand-over table): EVERY wave that stored results waits for its own stores to
  // complete -- __syncthreads() is s_waitcnt lgkmcnt(0) + s_barrier on gfx950 and does not wait on vmcnt -- and only
  // behind the barrier that follows does one lane count the workgroup in.  (inline asm: invisible to the waitcnt pass)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // every wave's write-through stores have completed (and the workgroup's LDS is free)
  if (threadIdx.x == 0) s_ticket = atomicAdd(&st.arrive, 1u);
  __syncthreads();
  if (s_ticket != expected_arrivals - 1u) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // nothing cached here predates the other workgroups' results
  p3p_replay<kSolver>(A, batch, single_mode, *reinterpret_cast<P3pReplayShared *>(smem_raw));
