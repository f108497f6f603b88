// the body of k_hamming_screen_mfma (hamming.hip): included by the kernel itself and by its gang form's Body::run, like
// hamming_screen.body.inc.  Same contract as k_hamming_screen, argument for argument; the distances come from the matrix
// cores: Hamming = (512 - <a', b'>) / 2 with the bits as e2m1 +-1 (k1_mfma_expand.h), 8 x
// v_mfma_scale_f32_32x32x64_f8f6f4 per 32 x 32 tile, exact in the f32 accumulators.
//
// One wave owns one 64-row bank block as two 32-row N tiles.  Lane l = 32 h + r holds, expanded once and kept for the
// whole query loop, dwords 8 h .. 8 h + 7 (planes 2 h, 2 h + 1 of the tiled64 bank) of rows r and 32 + r: 64 VGPRs.
// The query slice sits in LDS in bit form, one plane per 16 bytes of a row, so that the lane reads ITS dwords of query
// row q0 + r with two conflict-free 16-byte reads and expands them per use (7 VALU per MFMA step, each step feeding both
// N tiles).  With the bank rows on the N side a lane's 16 accumulators are 16 query rows of ONE bank row, so the
// running nearest is 8 x v_max3_f32 per tile.  Screening needs no index and no second neighbour beyond the head:
//   T = ratio_cnt[s1], s1 = second-nearest distance among the first `head` query rows (rounded up to whole 32-row
//   tiles: more rows give a smaller s1, still an upper bound of the query's second-nearest distance) -- the bound
//   k_hamming_screen starts from; it tightens it later, this kernel does not, so this flag set contains that one.
//   flag = (nearest distance over ALL query rows) < T.
// head_part must be null and gridDim.y 1 (the dispatch sends sliced scans to the popcount form).
  extern __shared__ uint4 qs[];  // [4 planes][lds_rows + 1]: the odd plane stride keeps the staging stores conflict free
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t r = lane & 31u, h = lane >> 5;
  const uint32_t w0 = blockIdx.x * WAVES + wave;
  const uint32_t blk = (w0 < n_work_blocks) ? (block_list ? block_list[w0] : w0) : kNoBlock;
  const bool valid = blk != kNoBlock;  // false also for the padding of a device-built list
  if (!__syncthreads_or(valid)) return;
  const uint32_t plane_stride = lds_rows + 1;
  const uint32_t plus_one = k1_mfma_plus_one_reg();
  v8i B[2][8];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (valid) v = bank[((uint64_t)blk * 4 + 2 * h + c) * 64 + 32 * t + r];
      B[t][4 * c + 0] = k1_mfma_operand(v.x, plus_one);
      B[t][4 * c + 1] = k1_mfma_operand(v.y, plus_one);
      B[t][4 * c + 2] = k1_mfma_operand(v.z, plus_one);
      B[t][4 * c + 3] = k1_mfma_operand(v.w, plus_one);
    }
  constexpr float kNoDot = -1024.f;  // below every dot product (-512 .. 512)
  float best[2] = {kNoDot, kNoDot};  // largest dot product = nearest query row, over all rows
  float hi1[2] = {kNoDot, kNoDot}, hi2[2] = {kNoDot, kNoDot};  // the two largest among the head rows (values only)
  const uint32_t head_rows = min(nq, (head + 31u) & ~31u);
  for (uint32_t j0 = 0; j0 < nq; j0 += lds_rows) {
    const uint32_t cnt = min(lds_rows, nq - j0);
    const uint32_t cnt_pad = (cnt + 31u) & ~31u;  // (the query buffer is zero padded to a multiple of 64 rows)
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < cnt_pad * 4; i += WAVES * 64)
      qs[(i & 3u) * plane_stride + (i >> 2)] = qdesc[(uint64_t)j0 * 4 + i];
    __syncthreads();
    if (!valid) continue;
    for (uint32_t jj = 0; jj < cnt_pad; jj += 32) {
      const uint4 a0 = qs[(2 * h) * plane_stride + jj + r], a1 = qs[(2 * h + 1) * plane_stride + jj + r];
      const uint32_t w[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      v16f c0 = {0}, c1 = {0};
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const v8i A = k1_mfma_operand(w[s], plus_one);
        c0 = k1_mfma_step(A, B[0][s], c0);
        c1 = k1_mfma_step(A, B[1][s], c1);
      }
      const uint32_t q0 = j0 + jj;
      if (q0 + 32 > nq) {  // the query's last tile: rows >= nq take no part
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
          if (q0 + (reg & 3) + 8 * (reg >> 2) + 4 * h >= nq) c0[reg] = kNoDot, c1[reg] = kNoDot;
      }
      if (q0 < head_rows) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          hi2[0] = __builtin_amdgcn_fmed3f(hi1[0], hi2[0], c0[reg]);
          hi1[0] = fmaxf(hi1[0], c0[reg]);
          hi2[1] = __builtin_amdgcn_fmed3f(hi1[1], hi2[1], c1[reg]);
          hi1[1] = fmaxf(hi1[1], c1[reg]);
        }
      }
#pragma unroll
      for (int reg = 0; reg < 16; reg += 2) {
        best[0] = fmaxf(fmaxf(best[0], c0[reg]), c0[reg + 1]);
        best[1] = fmaxf(fmaxf(best[1], c1[reg]), c1[reg + 1]);
      }
    }
  }
  if (!valid) return;
  // lanes l and l + 32 hold the two halves of the same bank rows' query rows: merge, then decide
  bool flag_t[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float o1 = __shfl_xor(hi1[t], 32, 64), o2 = __shfl_xor(hi2[t], 32, 64);
    hi2[t] = __builtin_amdgcn_fmed3f(hi1[t], hi2[t], o1);
    hi1[t] = fmaxf(hi1[t], o1);
    hi2[t] = __builtin_amdgcn_fmed3f(hi1[t], hi2[t], o2);
    best[t] = fmaxf(best[t], __shfl_xor(best[t], 32, 64));
    uint32_t T = 0;  // fewer than two head rows: no second neighbour, nothing can be accepted
    if (hi2[t] > -600.f) T = (uint32_t)ratio_cnt[k1_mfma_distance_of_dot((int)hi2[t])];
    flag_t[t] = (uint32_t)k1_mfma_distance_of_dot((int)best[t]) < T;
  }
  // back to one lane per bank row, as k_hamming_screen leaves it: bit (32 t + r) of the block's mask
  const unsigned long long mask =
      (__ballot(flag_t[0]) & 0xFFFFFFFFull) | ((unsigned long long)(__ballot(flag_t[1]) & 0xFFFFFFFFull) << 32);
  const bool flag = (mask >> lane) & 1ull;
  const uint32_t pidx = w0 * 64 + lane;
  if (lane == 0) {
    flagmask[w0] = mask;
    // (statistics: counters[0], the popcount form's finished pairs, stays 0 for this form)
    if (mask) atomicAdd(&counters[2u * (w0 & (uint32_t)(kK1CounterSlots - 1)) + 1], (unsigned long long)__popcll(mask));
  }
  if (mask) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(n_flagged, (uint32_t)__popcll(mask));
    base = __shfl(base, 0, 64);
    if (flag) {
      const uint32_t slot = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      flagged[slot] = make_uint2(pidx, blk * 64 + lane);
      // the exact pass wants the row compactly; this lane holds other rows' halves in expanded form, so the flagged
      // row (a fraction of a percent of the rows, its lines still in L2) is fetched again
      if (slot < flagged_desc_cap) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          flagged_desc[((uint64_t)(slot >> 6) * 4 + c) * 64 + (slot & 63u)] = bank[((uint64_t)blk * 4 + c) * 64 + lane];
      }
    }
  }
