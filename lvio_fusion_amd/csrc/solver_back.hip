// solver_back.hip — LM iteration, stage 4: back substitution of the dense corner and the sparse levels, the landmark back substitution
// and the candidate state x + dx; the merged last launch (k_chol_backsolve_tail) runs the last block step of stage 3 in front of them
// (its body: solver_dev.hpp).  Device code only (solver_args.hpp: argument blocks, constants, prototypes).
#include "solver_dev.hpp"

namespace lvf {

// workgroup barrier that orders LDS traffic only: __syncthreads() also drains vmcnt, i.e. it would wait for the global prefetches
// that are meant to stay in flight across it
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// back substitution x = L^-T y with y = augmented row L[d][0..d); ONE workgroup of 512 threads.  S points at the DENSE corner
// (row/column `off` of the full matrix), d = its unknowns, Dinv holds L_kk^-T of its 64x64 diagonal blocks.
// Nothing this kernel LOADS from global memory depends on x, so the chain is kept free of global latency:
//   * at entry every thread requests its share of the sparse levels' (row, owner, W[9]) items (registers) and the stored
//     L_bb^-1 (LDS): they arrive while the dense corner is being solved;
//   * dense corner, bottom-up:  rhs = y_blk - sum_{rows r below} L[r][blk]^T x_r  (thread (column c, part) takes rows part,
//     part + 8, ...), x_blk = Dinv_blk rhs (64x64 mat-vec split 8 ways); the gather operands and inverse block of the NEXT block
//     are prefetched while the current one is reduced;
//   * sparse levels in reverse, x_b = L_bb^-T (y_b - W_b^T x_N): the pre-loaded items are multiplied with x from LDS, summed per
//     block (wave-wide when a wave holds one block's rows, LDS atomics otherwise), one thread per (block, component) applies
//     L_bb^-1.  The solution leaves in the natural unknown order through `perm`.
// (S and Dinv are deliberately NOT __restrict__/invariant: LLVM would sink the prefetch loads past the barriers to their uses.)
template <typename T>
__device__ __forceinline__ T ld_off32(const T* base, unsigned byte_off) {     // wave-uniform base + 32-bit lane offset (saddr + voffset form)
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_off);
}
// LEVELS = false (the product form, k_backsolve_tail with Chain::back_product): the dense corner only.  The WHOLE dense-corner solution is
// published — the plan may leave (v, ba, bg) blocks in the corner's padding, and the sibling workgroups' product with G reads them — and the
// sparse items, the stored L_bb^-1 and the levels are neither requested nor run.
// XL (the back-substitution workgroup of k_chol_backsolve_tail; block form, LEVELS = false): the launch contains the last block step, so the
// first block is not solved here — nothing of it is requested — but read, behind a bounded wait, from what that step's inverse workgroup
// publishes (XLast); everything else the links need is final before the launch and in flight long before the flag goes up.
template <bool LEVELS = true, bool XL = false>
__device__ __forceinline__ void chol_backsolve_body(const BackArgs& A) {
  static_assert(!(XL && LEVELS), "the x_last entry exists beside the product form only");
  const int dv = done_flag_issue(A.done);
  const double* S = A.Sd; const int ld = A.ld, d = A.d; const double* Dinv = A.Dinv; double* xout = A.xout; const SpBack& sp = A.sp;
  extern __shared__ double sm[];          // xs[off] | x[nblk*64] | partial[kBParts][64] | rhs[64] | accs[9 max_count] | linv[81 n_nodes]
  const int tid = threadIdx.x, c = tid & 63, part = tid >> 6;
  const double* Tb = A.T;
  const bool blocks = Tb != nullptr;       // (where it is set nblk - 1 <= kBackTJ / kBackTJLevels and d is no multiple of 64, so the factor has nblk blocks: build_chain)
  const int nblk = (d + kNB - 1) / kNB, n = nblk * kNB;
  double* x = sm + sp.off;
  double* partial = x + n;
  double* rhs = partial + kBParts * kNB;
  double* accs = rhs + kNB;
  double* linv = accs + 9 * sp.max_count;
  double* part1 = linv + (sp.linv_in_lds ? 81 * sp.n_nodes : 0);     // [kBT] stage-1 partial sums
  double* prod = part1 + kBT;                                        // [prod_items][9]
  int* snode = reinterpret_cast<int*>(prod + 9 * (size_t)sp.prod_items);   // [n_nodes][2] = (row_off, m)
  int stamp = 0;
  auto mark = [&]() { if (sp.dbg && tid == 0) sp.dbg[stamp++] = wall_clock64(); };
  mark();
  // ---- dense corner
  const int rend = min(n, d);
  constexpr int kTJ = LEVELS ? kBackTJLevels : kBackTJ, kGl = kBackPre > 4 * kTJ * (kTJ + 1) ? kBackPre : 4 * kTJ * (kTJ + 1);
  double gl[kGl], xi[kBackInv], yv;        // gl: the gather operands of one block, or every block product of the block form
  // The kernel is ISSUE-bound (one workgroup, two waves per SIMD): every request below is a wave-uniform base (SALU) plus a 32-bit
  // per-lane byte offset, i.e. one VMEM instruction and no VALU address arithmetic, and the row tests are scalar branches -- with
  // 64-bit per-lane addresses and per-lane predicates issuing one block's 41 requests took 1.2-1.8 us of its 2.3-3.4.
  const int part_u = __builtin_amdgcn_readfirstlane(part);
  const unsigned c_off = 8u * (unsigned)c;
  // (no row tests either: k_prepare writes every entry of the padded corner, rows d.. meet x = 0, so the 8-row groups of the
  // 64 (nblk-1-kb) rows below a block are requested and multiplied whole)
  auto prefetch = [&](int kb) {
    const int r0 = kb * kNB, below = nblk - 1 - kb;
    const double* row = S + (size_t)(r0 + kNB + part_u) * ld + r0;
#pragma unroll
    for (int g = 0; g < kBackPre / 8; ++g)
      if (g < below) {
#pragma unroll
        for (int j = 0; j < 8; ++j) gl[8 * g + j] = ld_off32(row + (size_t)(kBParts * (8 * g + j)) * ld, c_off);
      }
    const double* dv = Dinv + (size_t)kb * kNB * kNB + kBackInv * part_u;
#pragma unroll
    for (int t = 0; t < kBackInv; ++t) xi[t] = ld_off32(dv + t, (unsigned)kNB * c_off);
    // the forward-substituted right-hand side: row d of the factor — a panel tile of S for every block but the last, whose part sits in
    // the factored DIAGONAL block (kept in the side buffer: chol_step_body)
    const double* yrow = (d / kNB == kb) ? A.Ldiag + (size_t)kb * kNB * kNB + (size_t)(d - r0) * kNB : S + (size_t)d * ld + r0;
    yv = (r0 + c < d) ? ld_off32(yrow, c_off) : 0.0;
  };
  if constexpr (!XL) prefetch(nblk - 1);
  // the stored L_bb^-1 and the node table go to LDS: ALL of a thread's requests are issued before the first LDS write (written as a
  // copy loop the compiler waits for every load in turn — eight dependent round trips at 50 keyframes, 4 of this kernel's 30 us)
  constexpr int kLinvPre = 8;
  if constexpr (LEVELS) {
  double lpre[kLinvPre];
  const int n_linv = sp.linv_in_lds ? 81 * sp.n_nodes : 0;
#pragma unroll
  for (int u = 0; u < kLinvPre; ++u) { const int i = tid + kBT * u; lpre[u] = i < n_linv ? ld_off32((const double*)sp.Linv, 8u * (unsigned)i) : 0.0; }
  SpNode ndpre = SpNode{0, 0, 0, 0};
  if (tid < sp.n_nodes) ndpre = sp.nodes[tid];
#pragma unroll
  for (int u = 0; u < kLinvPre; ++u) { const int i = tid + kBT * u; if (i < n_linv) linv[i] = lpre[u]; }
  for (int i = tid + kBT * kLinvPre; i < n_linv; i += kBT) linv[i] = sp.Linv[i];
  if (tid < sp.n_nodes) { snode[2 * tid] = ndpre.row_off; snode[2 * tid + 1] = ndpre.m; }
  for (int i = tid + kBT; i < sp.n_nodes; i += kBT) { const SpNode nd = sp.nodes[i]; snode[2 * i] = nd.row_off; snode[2 * i + 1] = nd.m; }
  asm volatile("" ::: "memory");
  }
  // block form: every link's share of T_kj, in the order the links run (k = j - 1, the one the next link waits for, first): all of it is in
  // flight while the first block is solved, and no link requests anything
  auto request_T = [&]() {
#pragma unroll
    for (int j = kTJ; j >= 1; --j)
      if (j < nblk) {
#pragma unroll
        for (int k = j - 1; k >= 0; --k) {
          const double* tb = Tb + ((size_t)k * nblk + j) * (kNB * kNB) + (size_t)(kBackInv * part_u) * kNB;
#pragma unroll
          for (int t = 0; t < kBackInv; ++t) gl[8 * (j * (j - 1) / 2 + k) + t] = ld_off32(tb + t * kNB, c_off);
        }
      }
  };
  if (blocks) request_T();
  // ---- requests for the sparse tail, AFTER the first dense prefetch: loads return in order, so the dense corner does not wait
  // for them and they land while it is being solved
  constexpr int kTailRegs = LEVELS ? kTailPre : 1;      // (the product form holds none of them)
  int tR[kTailRegs], tK[kTailRegs];
  double tW[kTailRegs][9];
#pragma unroll
  for (int u = 0; u < kTailRegs; ++u) {
    const int g = tid + kBT * u;
    const bool ok = LEVELS && g < sp.total_items;
    tR[u] = -1; tK[u] = 0;
#pragma unroll
    for (int q = 0; q < 9; ++q) tW[u][q] = 0.0;
    if (ok) {
      tR[u] = ld_off32((const int*)sp.rows, 4u * (unsigned)g);
      tK[u] = ld_off32((const int*)sp.owner, 4u * (unsigned)g);
#pragma unroll
      for (int q = 0; q < 9; ++q) tW[u][q] = ld_off32((const double*)sp.W, 8u * ((unsigned)q * (unsigned)sp.total_items + (unsigned)g));
    }
  }
  if (dv) return;                          // (every request above is in flight behind the flag's)
  for (int i = tid; i < sp.off + n; i += kBT) sm[i] = 0.0;
  lds_barrier();
  mark();
  if constexpr (XL) {
    // the bounded wait of wait_pose_ready (SpSrc has the rules): thread 0 polls, the workgroup meets at a barrier that leaves the T requests
    // in flight; on a time-out the hand-over flag is raised and the workgroup goes on — its consumers must see pose_ready either way
    if (tid == 0) {
      const unsigned long long t0 = wall_clock64();
      while (__hip_atomic_load((const int*)A.x_ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
        __builtin_amdgcn_s_sleep(4);
        if (wall_clock64() - t0 > (unsigned long long)A.x_timeout) { atomicMax((int*)A.x_fail, kFailHandover + 90001); break; }
      }
    }
    lds_barrier();
    mark();                                       // LVF_BACK_TIMING: the x_last flag was seen
    if (tid < kNB) x[(nblk - 1) * kNB + tid] = __hip_atomic_load((const double*)A.x_last + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    lds_barrier();
    mark();
  }
  const int kb_last = blocks ? nblk - 1 : 0;      // block form: the first solved block (its right-hand side sits in Ldiag) only
  for (int kb = nblk - 1; kb >= (XL ? nblk : kb_last); --kb) {
    const int r0 = kb * kNB;
    double s = 0.0;
#pragma unroll
    for (int g = 0; g < kBackPre / 8; ++g)
      if (g < nblk - 1 - kb) {
#pragma unroll
        for (int j = 0; j < 8; ++j) s += gl[8 * g + j] * x[r0 + kNB + part_u + kBParts * (8 * g + j)];
      }
    for (int r = r0 + kNB + part + kBParts * kBackPre; r < rend; r += kBParts) s += S[(size_t)r * ld + r0 + c] * x[r];
    partial[part * kNB + c] = s;
    double xc[kBackInv];
#pragma unroll
    for (int t = 0; t < kBackInv; ++t) xc[t] = xi[t];
    const double yc = yv;
    if (kb > kb_last) prefetch(kb - 1);    // in flight during the reductions below
    lds_barrier();
    if (part == 0) {
      double a = yc;
#pragma unroll
      for (int pp = 0; pp < kBParts; ++pp) a -= partial[pp * kNB + c];
      rhs[c] = a;
    }
    lds_barrier();
    double t2 = 0.0;
#pragma unroll
    for (int t = 0; t < kBackInv; ++t) t2 += xc[t] * rhs[kBackInv * part + t];
    partial[part * kNB + c] = t2;
    lds_barrier();
    if (part == 0) {
      double a = 0.0;
#pragma unroll
      for (int pp = 0; pp < kBParts; ++pp) a += partial[pp * kNB + c];
      // (block form: the multiplier carries -1 at the augmented row d, which meets column d - r0 of T_k,last = -Dinv_k y_k)
      x[r0 + c] = (r0 + c < d) ? a : ((blocks && r0 + c == d) ? -1.0 : 0.0);
    }
    lds_barrier();
    mark();
  }
  if (blocks) {
    // x_k = sum_{j > k} T_kj x_j: once x_j is in LDS every thread adds its eight terms for EVERY k < j to running sums; only block j - 1 is
    // reduced across the parts now — one write, two barriers and eight multiply-adds on the critical link
    double acc[kTJ];
#pragma unroll
    for (int k = 0; k < kTJ; ++k) acc[k] = 0.0;
#pragma unroll
    for (int j = kTJ; j >= 1; --j)
      if (j < nblk) {
        double xv[kBackInv];
#pragma unroll
        for (int t = 0; t < kBackInv; ++t) xv[t] = x[j * kNB + kBackInv * part_u + t];
#pragma unroll
        for (int k = j - 1; k >= 0; --k) {
#pragma unroll
          for (int t = 0; t < kBackInv; ++t) acc[k] += gl[8 * (j * (j - 1) / 2 + k) + t] * xv[t];
        }
        partial[part * kNB + c] = acc[j - 1];
        lds_barrier();
        if (part == 0) {
          double a = 0.0;
#pragma unroll
          for (int pp = 0; pp < kBParts; ++pp) a += partial[pp * kNB + c];
          x[(j - 1) * kNB + c] = a;
        }
        lds_barrier();
        mark();
      }
  }
  if (A.pose_ready) {
    // the pose increments are final (every pose row lives in the dense corner): out they go, so that the landmark back-substitution — which
    // reads nothing else of the step — runs in the sibling workgroups of this launch WHILE the sparse levels below are solved here
    // The increments and the flag travel as agent-scope ATOMICS (written through to the coherence point, read there by the consumers): an
    // agent-scope release / acquire FENCE pair instead writes this XCD's dirty L2 lines back and makes every consumer invalidate its L2 —
    // measured: 6 us on this workgroup's path and the landmark pass twice as long (320 workgroups flushing the E rows out of each other's
    // L2).  pose_fenced (LVF_CHAIN_FENCE=2) adds the fences back for A/B.
    {
      int last = -1;
      if constexpr (LEVELS) {
        for (int i = tid; i < A.n_pose; i += kBT) { __hip_atomic_store(xout + i, sm[sp.perm[i]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); last = i; }
      } else {
        // every unknown that lives in the dense corner: the poses and the (v, ba, bg) blocks the plan left there
        for (int i = tid; i < sp.d_total; i += kBT) {
          const int pi = sp.perm[i];
          if (pi >= sp.off) { __hip_atomic_store(xout + i, sm[pi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); last = i; }
        }
      }
      // (a store is acknowledged to the wave before it is necessarily performed; a load of the same address is ordered behind it and RETURNS:
      // once it is back — the s_waitcnt below — the store is where the consumers read.  Round 3 met the same with returnless atomic adds.)
      if (last >= 0) { const double chk = __hip_atomic_load(xout + last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); asm volatile("" ::"v"(chk)); }
    }
    if (A.pose_fenced) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");          // every wave's stores have been performed before the flag goes up
    if (tid == 0) __hip_atomic_store((int*)A.pose_ready, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if constexpr (!LEVELS) {
    mark();
    if (sp.dbg && tid == 0) sp.dbg[63] = (unsigned long long)stamp;
    return;
  }
  // ---- sparse levels, last eliminated first
  for (int lv = sp.lv.n - 1; lv >= 0; --lv) {
    const int first = sp.lv.first[lv], count = sp.lv.count[lv], item0 = sp.item0[lv], item1 = item0 + sp.items[lv];
    const bool staged = sp.items[lv] <= sp.prod_items;
    if (staged) {
      // (1) products -W x_r of every (block, row) item into LDS (stride 9 doubles: conflict-free)
#pragma unroll
      for (int u = 0; u < kTailRegs; ++u) {
        const int g = tid + kBT * u;
        if (g >= item0 && g < item1) {
          const double xr = (tR[u] == sp.aug) ? -1.0 : sm[tR[u]];          // the rhs row carries y_b itself
#pragma unroll
          for (int q = 0; q < 9; ++q) prod[9 * (g - item0) + q] = -tW[u][q] * xr;
        }
      }
      for (int g = max(item0, kBT * kTailPre) + tid; g < item1; g += kBT) {   // items beyond the register window (large windows only)
        const int R = sp.rows[g];
        const double xr = (R == sp.aug) ? -1.0 : sm[R];
#pragma unroll
        for (int q = 0; q < 9; ++q) prod[9 * (g - item0) + q] = -sp.W[(size_t)q * sp.total_items + g] * xr;
      }
      lds_barrier();
      // (2) thread (block k, component q, part j of J) sums its share of the block's rows; (3) thread (k, q) adds the J parts
      int J = 1;
      while (2 * J * 9 * count <= kBT && J < 32) J *= 2;
      if (tid < 9 * count * J) {
        const int j = tid % J, kq = tid / J, q = kq % 9, k = kq / 9;
        const int base = snode[2 * (first + k)] - item0, m = snode[2 * (first + k) + 1];
        double a = 0.0;
        for (int r = j; r < m; r += J) a += prod[9 * (base + r) + q];
        part1[tid] = a;
      }
      lds_barrier();
      if (tid < 9 * count) {
        double a = 0.0;
        for (int j = 0; j < J; ++j) a += part1[tid * J + j];
        accs[tid] = a;
      }
    } else {                                   // no LDS room for the products: LDS atomics (slow under contention, but general)
      for (int i = tid; i < 9 * count; i += kBT) accs[i] = 0.0;
      lds_barrier();
      for (int g = item0 + tid; g < item1; g += kBT) {
        const int R = sp.rows[g], k = sp.owner[g] - first;
        const double xr = (R == sp.aug) ? -1.0 : sm[R];
#pragma unroll
        for (int q = 0; q < 9; ++q) atomicAdd(&accs[9 * k + q], -sp.W[(size_t)q * sp.total_items + g] * xr);
      }
    }
    lds_barrier();
    for (int idx = tid; idx < 9 * count; idx += kBT) {
      const int kk = idx / 9, qq = idx - 9 * kk;
      double v = 0.0;                                       // x_q = sum_{t >= q} (L^-1)[t][q] acc_t
      if (sp.linv_in_lds) { const double* Li = linv + (size_t)(first + kk) * 81; for (int t = qq; t < 9; ++t) v += Li[t * 9 + qq] * accs[9 * kk + t]; }
      else { const double* Li = sp.Linv + (size_t)(first + kk) * 81; for (int t = qq; t < 9; ++t) v += Li[t * 9 + qq] * accs[9 * kk + t]; }
      sm[9 * (first + kk) + qq] = v;                        // block `first + kk` owns S columns 9 (first + kk) ..
    }
    lds_barrier();
    mark();
  }
  for (int i = tid; i < sp.d_total; i += kBT) xout[i] = sm[sp.perm[i]];
  mark();
  if (sp.dbg && tid == 0) sp.dbg[63] = (unsigned long long)stamp;
}
__global__ __launch_bounds__(kBT) void k_chol_backsolve(BackArgs a) { chol_backsolve_body(a); }
__global__ __launch_bounds__(kBT) void k_chol_backsolve_b(const BackArgs* __restrict__ t) { chol_backsolve_body(t[blockIdx.y]); }

// ------------------------------------------------------------------------------------------------ step pieces
// landmark back-substitution: dl = (-gr - e_l . dx_pose) / Cd ; model terms and norms
// (on DENSE rows one thread per landmark beat a wave per landmark, 25.6 vs 29.9 us; with the row limited to the landmark's track
// a per-thread walk diverges (41-54 us) and 16 lanes per landmark is the right shape)
// COH_DX: the pose increments were published by a sibling workgroup of THIS launch as agent-scope atomic stores: read past the non-coherent cache levels
// PRE > 0 (the landmark workgroups of k_backsolve_tail, which spend the dense solve waiting for the pose increments): nothing but the step
// depends on it, so the operands of the workgroup's first PRE passes are requested BEFORE `wait` (the bounded wait for the increments) — the
// track limits, then per lane a window of kLmEPre entries of the E band (16 lanes: 128 entries less the alignment slack, 18 keyframes; the
// tracks of synthetic.config4_window are geometric with mean 10) and gr / Cd / C / inv_depth.  Behind the wait these passes are the step
// into LDS, multiply-adds from registers, row16_sum and the stores; the rest of a longer band and any further pass are read as before.
// Two passes of 32 landmarks over 224 workgroups hold 14 336 landmarks: the 10 000 of the headline window need nothing else.
// (What is requested early is NOT __restrict__ then: LLVM would sink the requests past the wait to their uses, as in chol_backsolve_body.)
struct NoWait { __device__ __forceinline__ void operator()() const {} };
template <bool R, typename T> struct RestrictIf { typedef T* __restrict__ type; };
template <typename T> struct RestrictIf<false, T> { typedef T* type; };
template <int NT = kT, bool COH_DX = false, int PRE = 0, typename Wait = NoWait>
__device__ __forceinline__ void landmark_back_body(const int vb, const int nwg, int n_lm, int dp, int ldE, typename RestrictIf<PRE == 0, const double>::type E,
                                                   typename RestrictIf<PRE == 0, const double>::type C, typename RestrictIf<PRE == 0, const double>::type Cd,
                                                   typename RestrictIf<PRE == 0, const double>::type gr,
                                                   const double* __restrict__ dxc, typename RestrictIf<PRE == 0, const double>::type inv_depth,
                                                   double* __restrict__ dxl, double* __restrict__ invd2, double* __restrict__ scal,
                                                   typename RestrictIf<PRE == 0, const int>::type kmin, typename RestrictIf<PRE == 0, const int>::type kmax,
                                                   const Wait wait = Wait()) {
  extern __shared__ double sdx[];
  const int q = threadIdx.x & 15;
  constexpr int kP = PRE > 0 ? PRE : 1;
  int pb[kP], pi1[kP];
  double pe[kP][kLmEPre], pg[kP], pcd[kP], pc[kP], pid[kP];
  if constexpr (PRE > 0) {
#pragma unroll
    for (int p = 0; p < PRE; ++p) {
      const int l = vb * (NT / 16) + (threadIdx.x >> 4) + p * nwg * (NT / 16);
      const bool ok = l < n_lm;
      const int i0 = (ok && kmin) ? 6 * min(kmin[l], dp / 6) : 0;
      pi1[p] = ok ? (kmin ? 6 * (kmax[l] + 1) : dp) : 0;
      pb[p] = (i0 & ~15) + q;
      const double* e = E + (size_t)(ok ? l : 0) * ldE + pb[p];
#pragma unroll
      for (int u = 0; u < kLmEPre; ++u) pe[p][u] = pb[p] + 16 * u < pi1[p] ? e[16 * u] : 0.0;
      pg[p] = ok ? gr[l] : 0.0; pcd[p] = ok ? Cd[l] : 1.0; pc[p] = ok ? C[l] : 0.0; pid[p] = ok ? inv_depth[l] : 0.0;
    }
    // the values are consumed HERE, ahead of the wait: whatever the optimiser makes of the pointers, the requests cannot sink behind it
#pragma unroll
    for (int p = 0; p < PRE; ++p) {
#pragma unroll
      for (int u = 0; u < kLmEPre; ++u) asm volatile("" ::"v"(pe[p][u]));
      asm volatile("" ::"v"(pg[p]), "v"(pcd[p]), "v"(pc[p]), "v"(pid[p]));
    }
    wait();
  }
  for (int i = threadIdx.x; i < dp; i += NT) sdx[i] = COH_DX ? __hip_atomic_load(dxc + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : dxc[i];
  __syncthreads();
  // 16 lanes per landmark: the band of a row is a few 128-byte runs, read coalesced and reduced with four shuffles; the grid is
  // capped and strides over the landmarks so that the three scalar sums cost one atomic per WORKGROUP (thousands of per-wave
  // atomics on the 32 striped slots were most of this kernel's time)
  double m = 0.0, n2 = 0.0, x2 = 0.0, gmx = 0.0;
  if constexpr (PRE > 0) {
#pragma unroll
    for (int p = 0; p < PRE; ++p) {
      const int l = vb * (NT / 16) + (threadIdx.x >> 4) + p * nwg * (NT / 16);
      double ed = 0.0;
#pragma unroll
      for (int u = 0; u < kLmEPre; ++u) if (pb[p] + 16 * u < pi1[p]) ed += pe[p][u] * sdx[pb[p] + 16 * u];
      if (pb[p] + 16 * kLmEPre < pi1[p]) {        // the rest of a band longer than the window
        const double* e = E + (size_t)l * ldE;
        for (int i = pb[p] + 16 * kLmEPre; i < pi1[p]; i += 16) ed += e[i] * sdx[i];
      }
      ed = row16_sum(ed);
      if (q == 0 && l < n_lm) {
        const double g_l = pg[p];
        const double dl = (-g_l - ed) / pcd[p];
        gmx = fmax(gmx, fabs(g_l));
        dxl[l] = dl;
        invd2[l] = pid[p] + dl;
        m += -0.5 * dl * ((pcd[p] - pc[p]) * dl - g_l);
        n2 += dl * dl; x2 += pid[p] * pid[p];
      }
    }
  }
  for (int l = vb * (NT / 16) + (threadIdx.x >> 4) + PRE * nwg * (NT / 16); l < n_lm; l += nwg * (NT / 16)) {
    const double* e = E + (size_t)l * ldE;
    double ed = 0.0;
    const int i0 = kmin ? 6 * min(kmin[l], dp / 6) : 0, i1 = kmin ? 6 * (kmax[l] + 1) : dp;   // the row is zero outside the landmark's track
    for (int i = (i0 & ~15) + q; i < i1; i += 16) ed += e[i] * sdx[i];
    ed = row16_sum(ed);
    if (q == 0) {
      const double g_l = gr[l];
      const double dl = (-g_l - ed) / Cd[l];
      gmx = fmax(gmx, fabs(g_l));                   // Ceres' gradient_max_norm runs over every unknown, the inverse depths included
      dxl[l] = dl;
      invd2[l] = inv_depth[l] + dl;                 // the candidate inverse depth (was a second pass in k_apply_step)
      m += -0.5 * dl * ((Cd[l] - C[l]) * dl - g_l);
      n2 += dl * dl; x2 += inv_depth[l] * inv_depth[l];
    }
  }
  __shared__ double red[4][NT / 64];
  m = wave_sum(m); n2 = wave_sum(n2); x2 = wave_sum(x2);
  for (int o = 32; o > 0; o >>= 1) gmx = fmax(gmx, __shfl_down(gmx, o));
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = m; red[1][threadIdx.x >> 6] = n2; red[2][threadIdx.x >> 6] = x2; red[3][threadIdx.x >> 6] = gmx; }
  __syncthreads();
  if (threadIdx.x < 3) {
    double v = 0.0;
    for (int k = 0; k < NT / 64; ++k) v += red[threadIdx.x][k];
    double* dst = scal + (threadIdx.x == 0 ? SC_MODEL : (threadIdx.x == 1 ? SC_DXNORM : SC_XNORM));
    if (v != 0.0) atomicAdd(dst + (vb & (kStripes - 1)), v);
  } else if (threadIdx.x == 3) {
    double v = 0.0;
    for (int k = 0; k < NT / 64; ++k) v = fmax(v, red[3][k]);
    // (non-negative doubles order like their bit patterns; striped like the sums: hundreds of workgroups hitting ONE address serialise,
    // measured +4 us on this launch)
    if (v != 0.0) atomicMax(reinterpret_cast<unsigned long long*>(scal + SC_GMAX + (vb & (kStripes - 1))), (unsigned long long)__double_as_longlong(v));
  }
}
// Model cost change without a pass over H:  (H + D) dx = -g  =>  -dx^T (g + H dx / 2) = 1/2 sum_i dx_i (D_i dx_i - g_i).
// Camera part in k_apply_step (D_i = clamp(B_ii)/radius), landmark part in k_landmark_back.  SC_MODEL accumulates the NEGATED value
// (host flips the sign), keeping the convention model = -SC_MODEL.
// x_new = x [+] dx  (EigenQuaternionParameterization::Plus on the quaternion, plain add elsewhere)
// ... fused with the camera part of the model cost change (k_model_cam's body; d <= 15 n_kf threads of the same grid)
// PARTS: bit 0 = the pose unknowns (sums over [0, 6 n_kf), candidate poses), bit 1 = the (v, ba, bg) unknowns (sums over [6 n_kf, d), candidate
// velocities / biases); 3 = everything (k_step_tail).  k_backsolve_tail runs the two parts in different workgroups at different times.
// What apply_step_body reads for thread i (unknown i, keyframe i) that does not depend on the step: the pose workgroup of k_backsolve_tail
// requests it before it waits for the increments (the pointers are not __restrict__: the requests must stay where they are written).
struct StepOps { double h, h0d, gci, p[7]; int frozen, cm_kf; };
template <int PARTS>
__device__ __forceinline__ StepOps step_ops_load(const int i, int n_kf, StateP s, int d, int ld, const double* B, const double* gc,
                                                 const unsigned char* pose_const, const JacobiDev jac) {
  StepOps o{};
  if (i < d && ((PARTS & 1) || i >= 6 * n_kf) && ((PARTS & 2) || i < 6 * n_kf)) {
    o.h = B[(size_t)i * ld + i]; o.h0d = jac.h0[i]; o.gci = gc[i]; o.frozen = *jac.frozen;
  }
  o.cm_kf = (i < n_kf && pose_const) ? pose_const[i] : 0;      // bit 0: pose, bits 1..3: v, ba, bg held constant
  if (i < n_kf && (PARTS & 1)) {
    const double* sp = s.poses;
#pragma unroll
    for (int c = 0; c < 7; ++c) o.p[c] = sp[7 * i + c];
  }
  return o;
}
template <int NT = kT, int PARTS = 3>
__device__ __forceinline__ void apply_step_ops(const int vb, int n_kf, int n_lm, StateP s, const double* __restrict__ dxc, const double* __restrict__ dxl,
                                               double* __restrict__ poses2, double* __restrict__ vel2, double* __restrict__ ba2,
                                               double* __restrict__ bg2, double* __restrict__ invd2, double* __restrict__ scal, int d, double inv_radius,
                                               const StepOps& ops) {
  const int i = vb * NT + threadIdx.x;
  // step_norm / x_norm as Ceres takes them (trust_region_minimizer.cc): |x - x_plus_delta| and |x| over the AMBIENT parameter vector of the
  // reduced program — the quaternion's four coefficients, not its three tangent increments; constant pose blocks are not part of it
  double m = 0.0, n2 = 0.0, g = 0.0, x2 = 0.0;
  if (i < d && ((PARTS & 1) || i >= 6 * n_kf) && ((PARTS & 2) || i < 6 * n_kf)) {
    const double dx = dxc[i];
    const double h = ops.h, h0d = ops.h0d;
    m = -0.5 * dx * (lm_damping_fast(h, ops.frozen ? h0d : h) * inv_radius * dx - ops.gci);      // (first pass: H0 = H, being recorded by the assembly)
    const bool rot = i < 6 * n_kf && (i % 6) < 3;           // rotation increments enter through the quaternion difference below
    n2 = rot ? 0.0 : dx * dx;
    g = fabs(ops.gci);
  }
  const int cm_kf = ops.cm_kf;
  if (i < n_kf && (PARTS & 1)) {
    const double* p = ops.p; const double* dlt = dxc + 6 * i;
    const double nrm = sqrt(dlt[0] * dlt[0] + dlt[1] * dlt[1] + dlt[2] * dlt[2]);
    double* o = poses2 + 7 * i;
    if (nrm > 0.0) {
      const double sn = sin(nrm) / nrm, cw = cos(nrm);
      const double dx = sn * dlt[0], dy = sn * dlt[1], dz = sn * dlt[2];
      const double xw = p[3], xx = p[0], xy = p[1], xz = p[2];   // q_delta (x) x, Hamilton [w,x,y,z]
      o[3] = cw * xw - dx * xx - dy * xy - dz * xz;
      o[0] = cw * xx + dx * xw + dy * xz - dz * xy;
      o[1] = cw * xy - dx * xz + dy * xw + dz * xx;
      o[2] = cw * xz + dx * xy - dy * xx + dz * xw;
    } else { o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = p[3]; }
    for (int c = 0; c < 3; ++c) o[4 + c] = p[4 + c] + dlt[3 + c];
    for (int c = 0; c < 4; ++c) n2 += (o[c] - p[c]) * (o[c] - p[c]);
    if (!(cm_kf & 1)) for (int c = 0; c < 7; ++c) x2 += p[c] * p[c];
  }
  if (i < n_kf && (PARTS & 2)) {
    const int cm = cm_kf;
    const double* dv = dxc + 6 * n_kf + 9 * i;
    for (int c = 0; c < 3; ++c) { vel2[3 * i + c] = s.vel[3 * i + c] + dv[c]; ba2[3 * i + c] = s.ba[3 * i + c] + dv[3 + c]; bg2[3 * i + c] = s.bg[3 * i + c] + dv[6 + c]; }
    for (int c = 0; c < 3; ++c)
      x2 += ((cm & 2) ? 0.0 : s.vel[3 * i + c] * s.vel[3 * i + c]) + ((cm & 4) ? 0.0 : s.ba[3 * i + c] * s.ba[3 * i + c]) + ((cm & 8) ? 0.0 : s.bg[3 * i + c] * s.bg[3 * i + c]);
  }
  if (i < n_lm) invd2[i] = s.inv_depth[i] + dxl[i];
  if (vb * NT < d) {      // block-uniform
    block_add(m, scal + SC_MODEL); block_add(n2, scal + SC_DXNORM);
    for (int o = 32; o > 0; o >>= 1) g = fmax(g, __shfl_down(g, o));
    if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned long long*>(scal + SC_GMAX + (vb & (kStripes - 1))), (unsigned long long)__double_as_longlong(g));
  }
  block_add(x2, scal + SC_XNORM);
}
template <int NT = kT, int PARTS = 3>
__device__ __forceinline__ void apply_step_body(const int vb, int n_kf, int n_lm, StateP s, const double* __restrict__ dxc, const double* __restrict__ dxl,
                                                double* __restrict__ poses2, double* __restrict__ vel2, double* __restrict__ ba2,
                                                double* __restrict__ bg2, double* __restrict__ invd2, double* __restrict__ scal, int d, int ld,
                                                const double* __restrict__ B, const double* __restrict__ gc, double inv_radius,
                                                const unsigned char* __restrict__ pose_const, const JacobiDev jac) {
  const StepOps ops = step_ops_load<PARTS>(vb * NT + threadIdx.x, n_kf, s, d, ld, B, gc, pose_const, jac);
  apply_step_ops<NT, PARTS>(vb, n_kf, n_lm, s, dxc, dxl, poses2, vel2, ba2, bg2, invd2, scal, d, inv_radius, ops);
}

// landmark back-substitution and the camera-side step / model terms as ONE launch: workgroups [0, g_lm) walk the landmarks,
// the rest apply dx to the keyframe states (independent of the landmark results)
template <bool SEL = true> __device__ __forceinline__ const double* tail_E(const TailArgs& A) { return acc_set_t<SEL>(A.acc) ? (const double*)A.acc.E : (const double*)A.E; }
template <bool SEL = true> __device__ __forceinline__ const double* tail_B(const TailArgs& A) { return acc_set_t<SEL>(A.acc) ? (const double*)A.acc.B : (const double*)A.B; }
template <bool SEL = true> __device__ __forceinline__ const double* tail_gc(const TailArgs& A) { return acc_set_t<SEL>(A.acc) ? (const double*)A.acc.gc : (const double*)A.gc; }
template <bool SEL>
__device__ __forceinline__ void step_tail_body(const int bx, const TailArgs& A) {
  if (bx >= A.nblocks || (A.done && *A.done)) return;
  if (bx < A.g_lm) landmark_back_body(bx, A.g_lm, A.n_lm, A.dp, A.ldE, tail_E<SEL>(A), A.C, A.Cd, A.gr, A.dxc, A.s.inv_depth, A.dxl, A.invd2, A.scal, A.kmin, A.kmax);
  else apply_step_body(bx - A.g_lm, A.n_kf, 0, A.s, A.dxc, A.dxl, A.poses2, A.vel2, A.ba2, A.bg2, A.invd2, A.scal, A.d, A.ld, tail_B<SEL>(A), tail_gc<SEL>(A), 1.0 / *A.radius, A.pose_const, A.jac);
}
__global__ __launch_bounds__(kT) void k_step_tail(TailArgs a) { step_tail_body<true>(blockIdx.x, a); }
__global__ __launch_bounds__(kT) void k_step_tail_b(const TailArgs* __restrict__ t) { step_tail_body<false>(blockIdx.x, t[blockIdx.y]); }
__global__ __launch_bounds__(kT) void k_step_tail_bt(const TailArgs* __restrict__ t) { step_tail_body<false>(blockIdx.y, t[blockIdx.x]); }

// The back substitution and the step tail as ONE launch (single-window chain).  The landmark back-substitution needs the POSE part of the
// step only, and the poses are solved first (dense corner, 16 of the back substitution's 28 us); the sparse levels behind it (the
// velocities' and biases' increments, 11 us in one workgroup) and the landmark pass (10 us in hundreds of workgroups) have nothing to do
// with each other, yet as two launches they ran one after the other.  Here workgroup 0 is the back substitution — it publishes the pose
// increments as soon as the dense corner is done, goes on with the sparse levels and finally applies the step to the keyframe states
// (apply_step_body) — and workgroups 1.. are the landmark pass: they wait for the pose increments inside the launch (bounded, like the
// chained sparse levels: on a time-out the hand-over flag is raised, the pass is not judged and the host re-runs it with the two launches
// of old; SpSrc has the rules) and then walk the landmarks.  One launch boundary less and the two tails overlap: 39 -> 29 us at configs[3].
// Product form (g_prod > 0, Chain::back_product): workgroup 0 solves the dense corner only and publishes all of it; the (v, ba, bg) part of
// the step no longer runs behind it as five sequential levels but in g_prod further sibling workgroups, each owning kpw keyframes: they
// wait for the same flag as the landmark workgroups, take one product with their rows of G (formed under the dense factorisation:
// back_product_ride) and apply the (v, ba, bg) part of the step for their keyframes.  The launch then ends at flag + max(landmark pass,
// product) instead of flag + levels.
// the bounded wait of the consumers of pose_ready (SpSrc has the rules)
__device__ __forceinline__ void wait_pose_ready(const BackTailArgs& a) {
  if (threadIdx.x == 0) {
    const unsigned long long t0 = wall_clock64();
    while (__hip_atomic_load((int*)a.back.pose_ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
      __builtin_amdgcn_s_sleep(16);
      if (wall_clock64() - t0 > (unsigned long long)a.timeout_ticks) { atomicMax(a.fail, kFailHandover + 90000); break; }
    }
  }
  __syncthreads();
  if (a.fenced) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}
// G workgroup vb: keyframes [vb kpw, vb kpw + kpw).  Row (keyframe k, component c) is natural unknown dp + 9 k + c and S column perm[..]:
// below `off` it is G row perm[..] (an eliminated node), otherwise the block stayed in the dense corner and its increment is read from the
// published solution — either way it is applied here, exactly once.  16 lanes per row, 32 rows per pass; a lane's share of the first pass
// is requested into a fixed register window BEFORE the wait (what does not fit, and further passes, are read from memory afterwards).
constexpr int kGPre = 24, kLmPre = 2;      // kLmPre: passes of a landmark workgroup whose operands are requested before the wait (landmark_back_body)
// GW (k_chol_backsolve_tail): the riders that form the last level's rows of G run in the same launch — a bounded wait for their arrivals stands in
// front of the requests (long before the pose increments are due), and G is read with agent-scope atomic loads
template <bool GW = false>
__device__ __forceinline__ void back_product_body(const int vb, const BackTailArgs& a) {
  const TailArgs& T = a.tail; const SpBack& sp = a.back.sp;
  extern __shared__ double gsm[];          // xd[ldG]: [x_dense ; -1 ; 0 ..] | xs[9 kpw]: this workgroup's rows of the step
  double* xd = gsm; double* xs = gsm + a.ldG;
  const int tid = threadIdx.x, q = tid & 15, row = tid >> 4, ldG = a.ldG, nu = ldG >> 4;
  const int k0 = vb * a.kpw, nrows = 9 * min(a.kpw, T.n_kf - k0), i0 = T.dp + 9 * k0;      // the rows' natural unknowns are contiguous from i0
  unsigned long long* dbg = (sp.dbg && vb == 0 && tid == 0) ? sp.dbg + 40 : nullptr;
  if (dbg) dbg[0] = wall_clock64();
  auto ld_g = [](const double* p) { return GW ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p; };
  if constexpr (GW) {
    if (tid == 0 && a.g_target > 0) {
      const unsigned long long t0 = wall_clock64();
      while (__hip_atomic_load((const int*)a.g_ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < a.g_target) {
        __builtin_amdgcn_s_sleep(16);
        if (wall_clock64() - t0 > (unsigned long long)a.timeout_ticks) { atomicMax(a.fail, kFailHandover + 90002); break; }
      }
    }
    __syncthreads();
    if (dbg) dbg[5] = wall_clock64();      // LVF_BACK_TIMING: the riders of this launch have arrived
  }
  // ---- requests: nothing below depends on the step
  const int scol = row < nrows ? sp.perm[i0 + row] : -1;
  const bool in_g = scol >= 0 && scol < sp.off;
  const double* grow = a.G + (size_t)(in_g ? scol : 0) * ldG + q;
  double g[kGPre];
#pragma unroll
  for (int u = 0; u < kGPre; ++u) g[u] = (in_g && u < nu) ? ld_g(grow + 16 * u) : 0.0;
  const int ip0 = tid < ldG ? a.iperm[sp.off + tid] : -1;
  // the operands of this thread's unknown (thread t < nrows applies row t)
  const bool mine = tid < nrows;
  const int ui = i0 + (mine ? tid : 0), uk = k0 + (mine ? tid / 9 : 0), uc = mine ? tid % 9 : 0;
  const double* const Bt = tail_B(T); const double* const gct = tail_gc(T);
  const double* sv = uc < 3 ? (const double*)T.s.vel : (uc < 6 ? (const double*)T.s.ba : (const double*)T.s.bg);
  double* cv = uc < 3 ? (double*)T.vel2 : (uc < 6 ? (double*)T.ba2 : (double*)T.bg2);
  const double h = mine ? Bt[(size_t)ui * T.ld + ui] : 0.0, h0d = mine ? T.jac.h0[ui] : 0.0, gci = mine ? gct[ui] : 0.0;
  const double sval = mine ? sv[3 * uk + uc % 3] : 0.0;
  const int cm = (mine && T.pose_const) ? T.pose_const[uk] : 0;      // bit 0: pose, bits 1..3: v, ba, bg held constant
  const int frozen = *T.jac.frozen;
  const double inv_radius = 1.0 / *T.radius;
  if constexpr (GW) {
    // (consumed here: the requests cannot sink behind the wait, as in landmark_back_body)
#pragma unroll
    for (int u = 0; u < kGPre; ++u) asm volatile("" ::"v"(g[u]));
    if (dbg) dbg[6] = wall_clock64();      // LVF_BACK_TIMING: its share of G is in registers
  }
  wait_pose_ready(a);
  if (dbg) dbg[1] = wall_clock64();
  // ---- the dense solution, read at the coherence point
  for (int j = tid; j < ldG; j += kBT) {
    const int ip = j == tid ? ip0 : a.iperm[sp.off + j];
    xd[j] = ip >= 0 ? __hip_atomic_load(T.dxc + ip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (ip == -2 ? -1.0 : 0.0);      // (-2: the augmented column)
  }
  __syncthreads();
  if (dbg) dbg[2] = wall_clock64();
  // ---- rows of x
  {
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < kGPre; ++u) if (u < nu) s += g[u] * xd[q + 16 * u];
    if (in_g) for (int u = kGPre; u < nu; ++u) s += ld_g(grow + 16 * u) * xd[q + 16 * u];
    s = row16_sum(s);
    if (q == 0 && row < nrows) {
      if (in_g) { xs[row] = s; a.back.xout[i0 + row] = s; }      // (a block of the dense corner was written out by workgroup 0)
      else xs[row] = xd[scol - sp.off];
    }
  }
  for (int r0 = kBT / 16; r0 < nrows; r0 += kBT / 16) {             // further passes (more than 3 keyframes per workgroup)
    const int rw = r0 + row;
    const int sc = rw < nrows ? sp.perm[i0 + rw] : -1;
    const bool ing = sc >= 0 && sc < sp.off;
    double s = 0.0;
    if (ing) { const double* gr = a.G + (size_t)sc * ldG + q; for (int u = 0; u < nu; ++u) s += ld_g(gr + 16 * u) * xd[q + 16 * u]; }
    s = row16_sum(s);
    if (q == 0 && rw < nrows) {
      if (ing) { xs[rw] = s; a.back.xout[i0 + rw] = s; }
      else xs[rw] = xd[sc - sp.off];
    }
  }
  __syncthreads();
  if (dbg) dbg[3] = wall_clock64();
  // ---- the (v, ba, bg) part of the step for these keyframes: candidate state and the unknowns' share of the model cost change, the norms
  // and the gradient's max norm (apply_step_body's PARTS bit 1, one thread per unknown)
  double m = 0.0, n2 = 0.0, gm = 0.0, x2 = 0.0;
  if (mine) {
    const double dx = xs[tid];
    cv[3 * uk + uc % 3] = sval + dx;
    m = -0.5 * dx * (lm_damping_fast(h, frozen ? h0d : h) * inv_radius * dx - gci);
    n2 = dx * dx;
    gm = fabs(gci);
    x2 = (cm & (2 << (uc / 3))) ? 0.0 : sval * sval;
  }
  block_add(m, T.scal + SC_MODEL); block_add(n2, T.scal + SC_DXNORM); block_add(x2, T.scal + SC_XNORM);
  for (int o = 32; o > 0; o >>= 1) gm = fmax(gm, __shfl_down(gm, o));
  if ((tid & 63) == 0 && gm != 0.0) atomicMax(reinterpret_cast<unsigned long long*>(T.scal + SC_GMAX + (blockIdx.x & (kStripes - 1))), (unsigned long long)__double_as_longlong(gm));
  if (dbg) dbg[4] = wall_clock64();
}
// the pose workgroup of the merged launches: candidate poses and the pose unknowns' share of the model cost change / step norm (the
// increments are read at the coherence point into LDS; apply_step_ops takes them from there).  What the first 512 unknowns / keyframes read
// beside the increments — B's diagonal, h0, the gradient, the poses, the constant flags, the radius — is requested and consumed before the
// wait (a.early; LVF_BACK_EARLY=0: behind it, as it was).
__device__ __forceinline__ void back_tail_pose_body(const BackTailArgs& a) {
  const TailArgs& T = a.tail;
  extern __shared__ double sdx_pose[];
  const double* const Bt = tail_B(T); const double* const gct = tail_gc(T);
  StepOps ops{}; double radius = 0.0;
  if (a.early) {
    ops = step_ops_load<1>(threadIdx.x, T.n_kf, T.s, T.d, T.ld, Bt, gct, T.pose_const, T.jac);
    radius = *T.radius;
    asm volatile("" ::"v"(ops.h), "v"(ops.h0d), "v"(ops.gci), "v"(ops.frozen), "v"(ops.cm_kf), "v"(radius));
#pragma unroll
    for (int c = 0; c < 7; ++c) asm volatile("" ::"v"(ops.p[c]));
  }
  wait_pose_ready(a);
  for (int i = threadIdx.x; i < T.dp; i += kBT) sdx_pose[i] = __hip_atomic_load(T.dxc + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (!a.early) { ops = step_ops_load<1>(threadIdx.x, T.n_kf, T.s, T.d, T.ld, Bt, gct, T.pose_const, T.jac); radius = *T.radius; }
  const double inv_radius = 1.0 / radius;
  apply_step_ops<kBT, 1>(0, T.n_kf, 0, T.s, sdx_pose, T.dxl, T.poses2, T.vel2, T.ba2, T.bg2, T.invd2, T.scal, T.d, inv_radius, ops);
  for (int vb = 1; vb * kBT < max(T.dp, T.n_kf); ++vb)
    apply_step_body<kBT, 1>(vb, T.n_kf, 0, T.s, sdx_pose, T.dxl, T.poses2, T.vel2, T.ba2, T.bg2, T.invd2, T.scal, T.d, T.ld, Bt, gct, inv_radius, T.pose_const, T.jac);
  if (a.back.sp.dbg && threadIdx.x == 0) a.back.sp.dbg[62] = wall_clock64();      // LVF_BACK_TIMING: the pose part is applied
}
// landmark workgroup vb of a.g_lm of the merged launches (LVF_BACK_TIMING: the first and the last one leave their stamps)
__device__ __forceinline__ void back_tail_landmark_body(const int vb, const BackTailArgs& a) {
  const TailArgs& T = a.tail;
  unsigned long long* ldbg = (a.back.sp.dbg && (vb == 0 || vb == a.g_lm - 1) && threadIdx.x == 0) ? a.back.sp.dbg + (vb == 0 ? 56 : 59) : nullptr;
  if (ldbg) ldbg[0] = wall_clock64();
  if (a.early)
    landmark_back_body<kBT, true, kLmPre>(vb, a.g_lm, T.n_lm, T.dp, T.ldE, tail_E(T), T.C, T.Cd, T.gr, T.dxc, T.s.inv_depth, T.dxl, T.invd2, T.scal, T.kmin, T.kmax,
                                          [&]() { wait_pose_ready(a); if (ldbg) ldbg[1] = wall_clock64(); });
  else {
    wait_pose_ready(a);
    if (ldbg) ldbg[1] = wall_clock64();
    landmark_back_body<kBT, true>(vb, a.g_lm, T.n_lm, T.dp, T.ldE, tail_E(T), T.C, T.Cd, T.gr, T.dxc, T.s.inv_depth, T.dxl, T.invd2, T.scal, T.kmin, T.kmax);
  }
  if (ldbg) ldbg[2] = wall_clock64();
}
__global__ __launch_bounds__(kBT) void k_backsolve_tail(BackTailArgs a) {
  if (a.back.done && *a.back.done) return;                      // (every workgroup tests the same flag: nobody waits for a producer that has left)
  const TailArgs& T = a.tail;
  if (blockIdx.x == 0 && a.g_prod > 0) {
    chol_backsolve_body<false>(a.back);
    if (a.back.sp.dbg && threadIdx.x == 0) a.back.sp.dbg[55] = wall_clock64();      // LVF_BACK_TIMING: workgroup 0 is done
    return;
  }
  if ((int)blockIdx.x >= 2 + a.g_lm) { back_product_body((int)blockIdx.x - 2 - a.g_lm, a); return; }
  if (blockIdx.x == 0) {
    chol_backsolve_body(a.back);
    // the whole step is in xout (this workgroup wrote it): the velocities' and biases' part is applied here, with its share of the model cost
    // change.  (Requesting what that part reads — B's diagonal, the gradient, the states — ahead of the back substitution was measured
    // SLOWER: 36.1 vs 33.1 us for the launch; the registers it holds across the solve cost more than the three round trips it saves.)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    const double inv_radius = 1.0 / *T.radius;
    const double* const Bt = tail_B(T); const double* const gct = tail_gc(T);
    for (int vb = 0; vb * kBT < max(T.d, T.n_kf); ++vb)
      apply_step_body<kBT, 2>(vb, T.n_kf, 0, T.s, T.dxc, T.dxl, T.poses2, T.vel2, T.ba2, T.bg2, T.invd2, T.scal, T.d, T.ld, Bt, gct, inv_radius, T.pose_const, T.jac);
    if (a.back.sp.dbg && threadIdx.x == 0) a.back.sp.dbg[55] = wall_clock64();      // LVF_BACK_TIMING: the step is applied
    return;
  }
  if (blockIdx.x == 1) { back_tail_pose_body(a); return; }
  back_tail_landmark_body((int)blockIdx.x - 2, a);
}

// Block step nb - 1 and k_backsolve_tail as ONE launch (product and block forms, sub-block sweep; CholBackArgs has the roles).  Of the 12.5 us
// between the last pivot and pose_ready in two launches only the last block of the solution depends on the last diagonal block: the launch
// boundary, the back substitution's T requests and the consumers' own requests all run under the pivot sweep, which keeps two workgroups
// busy.  Producers carry the lowest workgroup numbers; nothing DEPENDS on that: every wait is bounded and raises the hand-over flag.  Every
// role tests `done` before anything else (the column workgroups and the riders inside their bodies), so nobody waits for a producer that left.
__global__ __launch_bounds__(kBT) void k_chol_backsolve_tail(CholBackArgs a) {
  static_assert(kCT == kBT, "one launch: the block step's workgroups and the back substitution's have the same size");
  const int bx = (int)blockIdx.x, kb = a.chol.nb - 1;
  if (bx < 2) { chol_step_body<true, true>(bx, a.chol, kb, a.xl); return; }
  const BackTailArgs& b = a.bt;
  if (bx == 2) {
    // T_{nb-2, nb-1} first (both factors are final since the launch before: no hand-off), on the kernel's panel buffers, in time that is
    // idle anyway; the requests of the body below read it back, hence the barrier and the workgroup-scope fences
    back_block_ride(0, a.chol, kb, a.tr);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    chol_backsolve_body<false, true>(b.back);
    if (b.back.sp.dbg && threadIdx.x == 0) b.back.sp.dbg[55] = wall_clock64();      // LVF_BACK_TIMING: the back substitution is done
    return;
  }
  if (bx < 3 + a.g.n) { back_product_ride<true>(bx - 3, a.g, a.g_arrive); return; }
  if (b.back.done && *b.back.done) return;
  const int role = bx - 3 - a.g.n;
  if (role == 0) back_tail_pose_body(b);
  else if (role <= b.g_prod) back_product_body<true>(role - 1, b);
  else back_tail_landmark_body(role - 1 - b.g_prod, b);
}

}  // namespace lvf
