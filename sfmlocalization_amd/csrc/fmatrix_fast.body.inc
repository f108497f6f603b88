// the body of k_fmatrix_fast (acransac.hip): included by the kernel itself and by its gang form's Body::run, so that
// the kernel compiles exactly as if the text stood in it (an inlined call does not: the loops are unrolled and scheduled
// before the inlining, and the scan lost 20 % that way)
  extern __shared__ unsigned char smem_raw[];
  F2Shared &S = *reinterpret_cast<F2Shared *>(smem_raw);
  const int tid = threadIdx.x;
  const int wv = tid >> 6, lane = tid & 63;
  STAMP_F_DECL;
  STAMP_F(1);
  const uint32_t v = A.view_sel ? A.view_sel[blockIdx.x] : blockIdx.x;
  if (A.merge.enabled) {  // K2 for this view (chain_device.h), by one wave; the others wait for its lists
    // The wide form: EVERY workgroup of the view builds the view's lists for itself and reads back what it wrote.  The
    // merge is one wave's deterministic work on inputs that no workgroup of this launch writes (flag words, partial
    // results), so the view's workgroups store the same values to the same places of match_i / match_key / view_count,
    // in whatever order: a workgroup that reads them after its own barrier finds those values whichever store landed
    // last, and nobody waits for anybody.  So that the ~97 of 100 listed views with nothing in them do not cost a merge
    // per workgroup, all but the first count the view's flagged rows first: the merge accepts flagged rows only, so
    // fewer of them than the smallest view this kernel takes proves that the view is not its own (the test below would
    // send this workgroup away with the same m).  The first workgroup always merges: later stages read view_count.
    if constexpr (kF2Wide) {
      if (blockIdx.y > 0 &&
          merge_flagged_rows_view(A.merge, blockIdx.x, (uint32_t)lane) < (uint32_t)(A.min_putative > 8 ? A.min_putative : 8))
        return;
    }
    if (wv == 0) merge_ratio_masked_view(A.merge, blockIdx.x, (uint32_t)lane);
    __syncthreads();
  }
  const int m = (int)A.put_count[v];
  const uint32_t off = A.view_off[v];
  constexpr int s = 7;
  if (m > kF2MaxM || m <= A.fast_min) return;  // another form's view (the larger fast form, k_fmatrix_filter) / done already
  if (m < A.min_putative || m <= s) {  // localization.cpp:408-415 ; ACRANSAC: nData <= sizeSample
    if (tid == 0 && (!kF2Wide || blockIdx.y == 0)) A.geo_count[v] = 0;
    return;
  }
  // NormalizePoints(x, w, h) for both images
  const int w1 = (int)A.view_wh[2 * v], h1 = (int)A.view_wh[2 * v + 1];
  const int w2 = (int)A.qw, h2 = (int)A.qh;
  const double s1 = 1.0 / sqrt((double)(w1 * h1)), s2 = 1.0 / sqrt((double)(w2 * h2));
  const double t1x = -0.5 * (double)w1 * s1, t1y = -0.5 * (double)h1 * s1;
  const double t2x = -0.5 * (double)w2 * s2, t2y = -0.5 * (double)h2 * s2;
  const double Dg = sqrt((double)w2 * (double)w2 + (double)h2 * (double)h2);
  const double Ar = (double)w2 * (double)h2;
  const double logalpha0 = det_log10(2.0 * Dg / Ar / s2);
  const double max_thr = (A.precision * A.precision) * s2 * s2;
  const double loge0 = det_log10(3.0 * (double)(m - s));
  const uint32_t stream = A.view_id[v];
  const int P = next_pow2(m);

  for (int p = tid; p < m; p += kF2Threads) {
    const uint32_t i = A.match_i[off + p];
    const uint32_t j = A.match_key[off + p] & 0xFFFFu;
    const float2 a = A.map_kpt[off + i];
    const float2 b = A.q_kpt6[j];
    S.pts[0][p] = s1 * (double)a.x + t1x;
    S.pts[1][p] = s1 * (double)a.y + t1y;
    S.pts[2][p] = s2 * (double)b.x + t2x;
    S.pts[3][p] = s2 * (double)b.y + t2y;
  }
  // logcombi tables (logcombi_tables_block is written for 256 threads); pre_models is free until the first batch
  logc_n_block(m, A.L10, &S.pre_models[0][0], S.logc_n, kF2Threads);
  for (int q = tid; q <= m; q += kF2Threads) {
    float val = 0.0f;
    if (s < q) {
      int k = s;
      if (q - k < k) k = q - k;
      double r = 0.0;
      for (int i = 1; i <= k; ++i) r += A.L10[q - i + 1] - A.L10[i];
      val = (float)r;
    }
    S.logc_k[q] = val;
  }
  __syncthreads();
  STAMP_F(2);  // prelude done (value: m in the low bits is not needed; the tool reads put_count)

  // (the lambdas below must not capture the kernel-argument struct: that would put all of it on the stack)
  const uint64_t seed = A.seed;
  F2Shared *const Sp = &S;
  // this wave: sample iteration `it`, solve, store the models at `models` / the count at *nm_out
  auto wave_solve = [Sp, seed, stream, lane](const int32_t *vec_index, int n_index, long it, double *models,
                                             int *nm_out) {
    F2Shared &S = *Sp;
    int32_t smp[7];
    ac_sample<7>(vec_index, n_index, seed, STAGE_FMATRIX, stream, (uint32_t)it, smp);
    const int r = lane / 9;
    int pidx = smp[0];
#pragma unroll
    for (int q = 1; q < 7; ++q)
      if (r == q) pidx = smp[q];
    double f = 0.0;
    const int nm = wave_seven_point(S.pts[0][pidx], S.pts[1][pidx], S.pts[2][pidx], S.pts[3][pidx], &f);
    if (lane < 9 * nm) models[lane] = f;
    if (lane == 0) *nm_out = nm;
  };
  // this wave: residuals of model M over all matches, sorted in registers, bestNFA; the sorted match indices go
  // to the wave's LDS segment (S.idx[wv]) for whoever needs the inlier list afterwards
  auto eval_e = [Sp, lane, wv, m, max_thr, logalpha0, loge0](const double *Mp, auto e_tag) -> NfaBest {
    constexpr int E = decltype(e_tag)::value;
    F2Shared &S = *Sp;
    double M[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) M[q] = Mp[q];
    uint64_t key[E];
    uint32_t idx[E];
#pragma unroll
    for (int r = 0; r < E; ++r) {
      const int p = (r << 6) + lane;
      uint64_t kv = ~0ull;
      if (p < m) kv = d2u(err_fmatrix(M, S.pts[0][p], S.pts[1][p], S.pts[2][p], S.pts[3][p]));
      key[r] = kv;
      idx[r] = (uint32_t)p;
    }
    uint32_t *iw = S.idx[wv];
    wave_sort_fast<E>(key, idx, iw);
#pragma unroll
    for (int r = 0; r < E; ++r) iw[(r << 6) + lane] = idx[r];
    return best_nfa_regs<E>(key, m, 7, max_thr, logalpha0, 0.5, loge0, S.logc_n, S.logc_k);
  };
  auto wave_eval = [&eval_e, P](const double *Mp) -> NfaBest {
    switch (P >> 6) {
      case 1: return eval_e(Mp, std::integral_constant<int, 1>{});
      case 2: return eval_e(Mp, std::integral_constant<int, 2>{});
      case 4: return eval_e(Mp, std::integral_constant<int, 4>{});
      default:
        if constexpr (kF2MaxM > kF2BigM) {
          if ((P >> 6) > 16) return eval_e(Mp, std::integral_constant<int, 32>{});
        }
        if constexpr (kF2MaxM > sfmloc::kF2MaxM) {  // (this instance's size against the base instance's, forms.h)
          if ((P >> 6) > 8) return eval_e(Mp, std::integral_constant<int, 16>{});
        }
        return eval_e(Mp, std::integral_constant<int, 8>{});
    }
  };

  // replicated scalar state (every thread holds the same values)
  double min_nfa = pos_inf();
  int n_in = 0;
  long n_iter = A.n_iter;
  long n_reserve = n_iter / 10;
  n_iter -= n_reserve;
  bool identity = true;
  bool inl_valid = true;  // S.best_inl holds the inliers of the best model (vacuously: n_in == 0)
  int n_index = m;
  long iter = 0;
  int best_mi = -1;  // S.best_model as a flattened model of the current batch, or -1: it came from an earlier one

  // wave 0 rebuilds the inlier list of S.best_model into best_inl (and vec_index when `to_index`)
  auto rebuild_inliers = [&wave_eval, Sp, wv, lane, &n_in](bool to_index) {
    F2Shared &S = *Sp;
    __syncthreads();
    if (wv == 0) {
      (void)wave_eval(S.best_model);
      if (lane == 0) S.idx_model[0] = -1;  // (wave 0's segment holds this list now, no model of the batch's)
      wave_lds_sync();
      for (int p = lane; p < n_in; p += 64) {
        const int32_t q = (int32_t)S.idx[0][p];
        S.best_inl[p] = q;
        if (to_index) S.vec_index[p] = q;
      }
    }
    __syncthreads();
  };
  // The inlier list of the batch's flattened model `mi`, which has just become S.best_model (mi < 0: of an earlier
  // batch's).  The wave that evaluated it left exactly that list -- the same function on the same inputs -- in its
  // segment of S.idx; unless that wave has evaluated another model since, every thread copies from there.  Otherwise,
  // and always for the wide form's first batch, which other workgroups evaluated: rebuild_inliers.
  auto take_inliers = [&rebuild_inliers, Sp, tid, &n_in](int mi, bool to_index) {
    F2Shared &S = *Sp;
    int owner = -1;
    if (mi >= 0)
      for (int w = 0; w < kF2Waves; ++w)
        if (S.idx_model[w] == mi) owner = w;
    if (tid == 0) k3_count_list(owner >= 0);
    if (owner < 0) {
      rebuild_inliers(to_index);
      return;
    }
    for (int p = tid; p < n_in; p += kF2Threads) {
      const int32_t q = (int32_t)S.idx[owner][p];
      S.best_inl[p] = q;
      if (to_index) S.vec_index[p] = q;
    }
    // (no barrier: nothing reads the two lists, or writes a segment of S.idx, before the next batch's first barrier or
    // the one behind the loop)
  };

  // The WIDE form (a query alone on the GPU): gridDim.y workgroups per view, one per iteration of the first uniform batch.
  // Each solves its iteration and evaluates the iteration's models, one wave each, on a compute unit of its own -- in the
  // plain form the batch's 23 solves and ~50 evaluations share ONE compute unit's four SIMDs, 105 of a lone headline
  // query's 150 us in this kernel --, delivers the results (write-through stores, as a round of K5 does) and counts itself
  // in; the workgroup that arrives last takes the results of all of them, replays the sequential rule over them and goes
  // on alone with whatever iterations follow.  Nobody waits for anybody; same samples, same arithmetic, same replay.
  bool first_batch_done = false;
  if constexpr (kF2Wide) {
    const int B0 = (int)gridDim.y;  // (the host's min(n_iter, kF2Batch): the first batch of the loop below)
    K3Spec *const spec_v = A.spec + (size_t)blockIdx.x * kF2Batch;
    {
      const int b = (int)blockIdx.y;
      if (wv == 0) wave_solve(nullptr, m, (long)b, S.pre_models[0], &S.pre_nm[0]);
      __syncthreads();
      const int nm = S.pre_nm[0];
      K3Spec *const out = spec_v + b;
      if (wv < nm) {
        const NfaBest r = wave_eval(&S.pre_models[0][9 * wv]);
        if (lane < 9) store_through(&out->models[9 * wv + lane], S.pre_models[0][9 * wv + lane]);
        if (lane == 0) {
          store_through(&out->nfa[wv], r.nfa);
          store_through(&out->k[wv], r.k);
        }
      }
      if (tid == 0) store_through(&out->nm, nm);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (every storing wave: p3p_round.body.inc's producer rule)
    __syncthreads();
    if (tid == 0) S.wide_ticket = atomicAdd(&A.spec_arrive[blockIdx.x], 1u);
    __syncthreads();
    if (S.wide_ticket != gridDim.y - 1u) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // nothing cached here predates the other workgroups' results
    if (tid == 0) A.spec_arrive[blockIdx.x] = 0u;       // the view slot's next query counts from zero
    for (int q = tid; q < B0 * 27; q += kF2Threads) S.pre_models[q / 27][q % 27] = spec_v[q / 27].models[q % 27];
    for (int q = tid; q < B0 * 3; q += kF2Threads) {
      S.res_nfa[q / 3][q % 3] = spec_v[q / 3].nfa[q % 3];
      S.res_k[q / 3][q % 3] = spec_v[q / 3].k[q % 3];
    }
    for (int q = tid; q < B0; q += kF2Threads) S.pre_nm[q] = spec_v[q].nm;
    first_batch_done = true;  // (the barrier at the head of the loop's first batch orders these writes)
  }

  // Every iteration is taken in speculative batches: the batch's samples are drawn as if no iteration of it changed the
  // set they are drawn from, its models are solved and evaluated in parallel, and the sequential rule is replayed over
  // them in order; the replay closes the batch at the first iteration that DOES change the set (the end of the uniform
  // phase; afterwards every better model: its inliers become the set), and the iterations behind it are drawn again.
  // While sampling is uniform a batch is kF2Batch iterations; from the inlier set -- where a better model, i.e. a new
  // set, comes every ten iterations or so -- one per wave.  (Until round 4 the iterations after the uniform phase went one
  // at a time, one wave solving and at most three evaluating: the reserve's ~100 iterations were 0.45 of a lone image
  // frame's 0.48 ms in this kernel.)
  while (iter < n_iter) {
    const long cap = identity ? (long)kF2Batch : (long)(kF2Waves < kF2Batch ? kF2Waves : kF2Batch);
    const int B = (int)((n_iter - iter < cap) ? (n_iter - iter) : cap);
    const int32_t *const sample_from = identity ? nullptr : S.vec_index;
    const int n_from = identity ? m : n_index;
    __syncthreads();  // pre_* / res_* of the previous batch are no longer read
    if (tid < kF2Waves) S.idx_model[tid] = -1;  // flattened indices count from zero again: no segment holds a model of this batch
    best_mi = -1;
    if (!first_batch_done)
      for (int b = wv; b < B; b += kF2Waves) wave_solve(sample_from, n_from, iter + b, S.pre_models[b], &S.pre_nm[b]);
    __syncthreads();
    STAMP_F(3);  // speculative solves done
    // flattened model list in iteration order
    if (tid == 0) {
      int n = 0;
      for (int b = 0; b < B; ++b) {
        for (int k = 0; k < S.pre_nm[b]; ++k) {
          S.flat_b[n] = (uint8_t)b;
          S.flat_k[n] = (uint8_t)k;
          ++n;
        }
        S.iter_end[b] = n;
      }
    }
    __syncthreads();
    const int total = S.iter_end[B - 1];
    // evaluate the models eight per round; before each round replay the iterations whose models are all done,
    // and stop as soon as one of them ends the uniform phase
    int done = first_batch_done ? total : 0;  // models evaluated so far (the wide form's first batch: all of them)
    first_batch_done = false;
    int b_done = 0;  // iterations replayed so far
    bool stop = false;
    for (;;) {
      while (b_done < B && S.iter_end[b_done] <= done) {
        const int b = b_done;
        bool better = false;
        int bk = -1;
        for (int k = 0; k < S.pre_nm[b]; ++k)
          if (S.res_nfa[b][k] < min_nfa) {
            better = true;
            min_nfa = S.res_nfa[b][k];
            n_in = S.res_k[b][k];
            bk = k;
          }
        if (better) {
          inl_valid = false;
          if (tid < 9) S.best_model[tid] = S.pre_models[b][9 * bk + tid];
          best_mi = (b ? S.iter_end[b - 1] : 0) + bk;
        }
        ++b_done;
        const long it = iter + b;
        if ((better && min_nfa < 0.0) || (it + 1 == n_iter && n_reserve)) {
          if (n_in == 0) {
            n_iter++;
            n_reserve--;  // the iteration budget moved: close this batch here
          } else {
            STAMP_F(6);  // the sampled set changes: the new set's sorted list is fetched (7: there)
            take_inliers(best_mi, true);
            STAMP_F(7);
            inl_valid = true;
            n_index = n_in;
            identity = false;
            if (n_reserve) {
              n_iter = it + 1 + n_reserve;
              n_reserve = 0;
            }
          }
          stop = true;
          break;
        }
      }
      if (stop || b_done >= B) break;
      const int mi = done + wv;
      if (mi < total) {
        const int bb = S.flat_b[mi], kk = S.flat_k[mi];
        const NfaBest r = wave_eval(&S.pre_models[bb][9 * kk]);
        if (lane == 0) {
          S.idx_model[wv] = mi;  // (this wave's segment of S.idx: that model's sorted matches, until it evaluates again)
          S.res_nfa[bb][kk] = r.nfa;
          S.res_k[bb][kk] = r.k;
        }
      }
      __syncthreads();
      STAMP_F(4);  // one evaluation round done
      done = (done + kF2Waves < total) ? done + kF2Waves : total;
    }
    STAMP_F(5);  // batch closed (incl. the inlier rebuild when the sampled set changed)
    iter += b_done;
  }
  __syncthreads();
  STAMP_F(8);
  if (min_nfa >= 0.0) n_in = 0;
  if ((double)n_in > 7 * 2.5) {
    if (!inl_valid) {
      STAMP_F(6);
      take_inliers(best_mi, false);
      STAMP_F(7);
    }
    for (int p = tid; p < n_in; p += kF2Threads) A.geo_idx[off + p] = (uint32_t)S.best_inl[p];
    if (tid == 0) A.geo_count[v] = (uint32_t)n_in;
    __syncthreads();
    if (A.geo_model && tid == 0) {  // errorMax = the residual of the last inlier (the list ascends by residual)
      const int pl = S.best_inl[n_in - 1];
      double Mb[9];
      for (int q = 0; q < 9; ++q) Mb[q] = S.best_model[q];
      double *gm = A.geo_model + 10 * (size_t)v;
      for (int q = 0; q < 9; ++q) gm[q] = Mb[q];
      gm[9] = err_fmatrix(Mb, S.pts[0][pl], S.pts[1][pl], S.pts[2][pl], S.pts[3][pl]);
    }
  } else if (tid == 0) {
    A.geo_count[v] = 0;
  }
  STAMP_F(9);
