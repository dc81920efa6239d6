// solver_assemble.hip — LM iteration, stage 2: from the accumulators of a linearisation to the damped reduced camera system.  Slab
// reduction, damping, Schur elimination of the 1x1 inverse-depth blocks (MFMA f64; dense, LDS and band-limited forms), the landmark-track
// and slot layout kernels of problem_configure, and the sparse (v, ba, bg) levels that ride in these launches.
//
// Unknown ordering (reduced system, d = 15 n_kf):  [ pose tangent 6 x n_kf | (v, ba, bg) 9 x n_kf ].
// H = [B E^T; E C], C diagonal (one inverse depth per landmark).  LM step: (H + D^2/radius) dx = -g with
// D^2 = clamp(diag H, 1e-6, 1e32).  S = B + Dc - E^T diag(1/(C + Dl)) E touches only the pose-pose corner, so E is
// kept dense [n_lm x ldE] (ldE = 6 n_kf rounded up to 16, +1 column carrying g_rho) and the rank-n_lm update is one
// v_mfma_f64_16x16x4_f64 SYRK ("MFMA only for the dense Schur reduce").  The right-hand side rides along as an
// augmented ROW of S (index d), so the forward substitution comes out of the Cholesky for free.
// Device code only (solver_args.hpp: argument blocks, constants, prototypes); sp_ride and sp_eliminate_body are private to this unit:
// every launch a sparse level rides in (k_tf_reduce*, k_prepare*, k_schur_sp0*) is defined here.
#include "solver_dev.hpp"

namespace lvf {

// ------------------------------------------------------------------------------------------------ damping
// (lm_damping_fast: solver_dev.hpp)
// the damping of unknown `slot` whose diagonal entry is h in this pass; the thread that OWNS the entry's assembly records H0 in the first
// pass.  h0_loaded = jac.h0[slot], requested by the caller together with its other loads (so that it is not a dependent round trip here).
__device__ __forceinline__ double lm_damping_fast_own(double h, const JacobiDev& j, int slot, int frozen, double h0_loaded) {
  double h0 = h0_loaded;
  if (!frozen) { h0 = h; j.h0[slot] = h; }
  return lm_damping_fast(h, h0);
}

// ------------------------------------------------------------------------------------------------ elimination order
// The (v, ba, bg) blocks only meet each other and the poses through ImuError factors, i.e. along the IMU chain: block k touches
// blocks k-1, k+1 and poses k-1, k, k+1.  Factorising them FIRST, in nested-dissection order (level 0 = every other block of the
// chain, level 1 = every other one of what is left, ...; any coupling graph works, the levels are greedy independent sets with
// fill-in tracked on the host), costs 9 sequential pivots per LEVEL instead of 9 per block, and leaves only the pose corner
// (6 n_kf) for the dense blocked factorisation: at 50 keyframes 6 x 9 + 300 sequential pivots instead of 750.
// k_sp_eliminate, one launch per level, `tiles` workgroups per block b with neighbour rows N (|N| = m):
//   L_bb = chol(S_bb) (wave 0, lane = row, pivots broadcast by v_readlane);  W = S_Nb L_bb^-T (thread per row);
//   S_NN -= W W^T (pairs split over the tiles; atomics, because blocks of one level share neighbours).
// W and L_bb go to side buffers (the eliminated columns of S are never read again), so the tiles of a block never race.
__device__ __forceinline__ void sp_eliminate_body(const int vb, const SpNode* __restrict__ nodes, int first, int tiles, const int* __restrict__ rows,
                                                  double* __restrict__ S, int ld, double* __restrict__ W, int wstride,
                                                  double* __restrict__ Lout, int* __restrict__ fail, const int* done = nullptr,
                                                  const SpSrc src = SpSrc{nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 1, 200000u, 0, 0, nullptr, 0}) {
  extern __shared__ double sp_sm[];        // Ws[m][9] | L[81] | linv[9] | rws[m] (int) | rnat[m] (int, early form)
  const int dv = done_flag_issue(done);
  const int ni = first + vb / tiles, tile = vb % tiles, tid = threadIdx.x;
  unsigned long long* stamp = (src.dbg && tile == 0 && tid == 0) ? src.dbg + (size_t)ni * 8 : nullptr;
  if (stamp) stamp[0] = wall_clock64();
  const SpNode nd = nodes[ni];
  const double radius = src.B ? *src.radius : 1.0;
  if (dv) return;
  const bool chained = src.wait_counter != nullptr;
  // an entry of S the level below may have added into during THIS launch: an agent-scope atomic load behind the acquire fence that
  // follows the wait (the adds it must see were RETURNING atomics performed before the producer's release arrival; the wrong results
  // round 3 chased — 5 of 12 runs of the 8-keyframe / 20 000-landmark case — came from RETURNLESS adds on the producer side, not from
  // this load).  rmw_read (LVF_CHAIN_RMW_READ=1, diagnostic): a returning atomic adding zero instead — same results, 7 us slower.
  auto ld_s = [&](double* ptr) -> double {
    if (!chained) return *ptr;
    return src.rmw_read ? __hip_atomic_fetch_add(ptr, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : __hip_atomic_load(ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  const int m = nd.m, col = nd.col;
  double* Ws = sp_sm;
  double* L = sp_sm + 9 * m;
  double* linv = L + 81;
  int* rws = reinterpret_cast<int*>(linv + 9);
  int* rnat = rws + m;
  const int nb0 = src.dp + 9 * nd.id;      // early form: the block's first unknown in the natural order (poses | 9 per keyframe)
  // The level is a chain of dependent round trips (node -> row list -> rows -> factor -> W -> updates), so everything is requested as early
  // as its address is known, and the rows are dealt to waves 1..3 first: their requests are in flight while wave 0 factors the block
  // (wave 0 only takes rows when there are more than 192).  Each thread keeps its FIRST row in registers; further rows (m > 256) follow
  // the classic loop behind the barrier.
  const int r0 = (tid + 192) & 255;
  // ---- phase A: what does not depend on the level below
  const bool has0 = r0 < m;
  int rw0 = 0, rn0 = -1;
  if (has0) { rw0 = rows[nd.row_off + r0]; if (src.B) rn0 = src.rows_nat[nd.row_off + r0]; }
  for (int r = tid; r < m; r += 256) { rws[r] = rows[nd.row_off + r]; if (src.B) rnat[r] = src.rows_nat[nd.row_off + r]; }
  double bd[9], sv0[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) { bd[c] = 0.0; sv0[c] = 0.0; }
  if (src.B) {
    if (tid < 9) {                         // what k_prepare would have stored in the diagonal block: B + clamp(diag B) / radius
      const double inv_radius = 1.0 / radius;
      const int jf = *src.jac.frozen;
      const double h0d = src.jac.h0[nb0 + tid];
      // (the row's nine entries are requested together, column clamped to the diagonal: as `c <= tid ? B[..] : 0` each load sat behind its own
      // branch and was waited for there — nine dependent round trips at the head of every sparse level)
      double braw[9];
#pragma unroll
      for (int c = 0; c < 9; ++c) braw[c] = src.B[(size_t)(nb0 + tid) * src.ldB + nb0 + min(c, tid)];
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        double b = c <= tid ? braw[c] : 0.0;
        if (c == tid) b += lm_damping_fast_own(b, src.jac, nb0 + tid, jf, h0d) * inv_radius;      // (every tile workgroup of the node stores the same H0)
        bd[c] = b;
      }
    }
    if (has0) {                            // the row's entries of B (lower triangle, natural order) / of -gc (the right-hand-side row)
      if (rn0 == -2) {
#pragma unroll
        for (int c = 0; c < 9; ++c) sv0[c] = -src.gc[nb0 + c];
      } else if (rn0 >= 0) {
#pragma unroll
        for (int c = 0; c < 9; ++c) { const int oj = nb0 + c; sv0[c] = src.B[(size_t)max(rn0, oj) * src.ldB + min(rn0, oj)]; }
      }
    }
  }
  if (stamp) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp[1] = wall_clock64(); }      // (timing only: phase A's requests have landed)
  if (chained) {
    // bounded: if the level below does not arrive in time (workgroups of another stream or process took the CUs its producers needed, or
    // a dispatch order this code does not expect) the hand-over flag is raised instead of hanging; the step is then NOT judged: see SpSrc
    if (tid == 0) {
      const unsigned long long t0 = wall_clock64();
      while (__hip_atomic_fetch_add((int*)src.wait_counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < src.wait_target) {
        __builtin_amdgcn_s_sleep(4);
        if (wall_clock64() - t0 > (unsigned long long)src.timeout_ticks) { atomicMax(fail, kFailHandover + nd.id); break; }
      }
    }
    asm volatile("s_barrier" ::: "memory");           // (not __syncthreads(): the requests above stay in flight across it)
    // every wave orders its reads of S behind the producers' release arrivals (agent scope: the L1 copy of a line an earlier level's
    // plain loads brought in is dropped; phase A's requests have long landed while the wave sat at the barrier)
    if (src.fenced) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  if (stamp) stamp[2] = wall_clock64();
  // ---- phase B: what the level below added into S
  double a[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) a[c] = 0.0;
  if (tid < 9) {
    double sraw[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) sraw[c] = 0.0;
    if (!src.s_zero) {                      // (all nine requested together, column clamped to the diagonal: see phase A)
#pragma unroll
      for (int c = 0; c < 9; ++c) sraw[c] = ld_s(&S[(size_t)(col + tid) * ld + col + min(c, tid)]);
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) a[c] = (c <= tid ? sraw[c] : 0.0) + bd[c];
  }
  if (has0 && !src.s_zero) {
    double* srow = S + (size_t)rw0 * ld + col;
#pragma unroll
    for (int c = 0; c < 9; ++c) sv0[c] += ld_s(srow + c);
  }
  if (stamp) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp[3] = wall_clock64(); }      // (timing only: the S entries are here)
  if (tid < 64) {
    const int lane = tid;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const double djj = lane_bcast(a[j], j);
      bad |= !(djj > 0.0);
      // hardware estimate + one second-order correction (as in the dense corner); lane j holds A_jj itself, so no select
      const double y0 = __builtin_amdgcn_rsq(djj);
      const double e = fma(-djj * y0, y0, 1.0);
      const double inv_l = fma(y0 * e, fma(e, 0.375, 0.5), y0);
      a[j] *= inv_l;
      if (lane == j) linv[j] = inv_l;
      // A_rt -= L_rj L_tj (meaningful for t <= r): L_tj sits in lane t of the same 16-lane row — the DPP row broadcast hands it to the
      // multiply-add directly (one instruction per column instead of two v_readlane + one FMA)
      {
        const double m = -a[j];
        asm volatile("s_nop 4");
        if (j < 1) fmac_row_bcast<1>(a[1], a[j], m);
        if (j < 2) fmac_row_bcast<2>(a[2], a[j], m);
        if (j < 3) fmac_row_bcast<3>(a[3], a[j], m);
        if (j < 4) fmac_row_bcast<4>(a[4], a[j], m);
        if (j < 5) fmac_row_bcast<5>(a[5], a[j], m);
        if (j < 6) fmac_row_bcast<6>(a[6], a[j], m);
        if (j < 7) fmac_row_bcast<7>(a[7], a[j], m);
        if (j < 8) fmac_row_bcast<8>(a[8], a[j], m);
      }
    }
    if (lane < 9) {
#pragma unroll
      for (int c = 0; c < 9; ++c) L[lane * 9 + c] = (c <= lane) ? a[c] : 0.0;
    }
    if (bad && lane == 0) atomicMax(fail, kFailSparse + nd.id);
  }
  if (stamp) stamp[4] = wall_clock64();
  __syncthreads();
  auto finish_row = [&](const int r, const double sv[9]) {     // W_r = S_rb L_bb^-T
    double w[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      double v = sv[c];
#pragma unroll
      for (int k = 0; k < c; ++k) v -= w[k] * L[c * 9 + k];
      w[c] = v * linv[c];
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) Ws[r * 9 + c] = w[c];
    if (tile == 0) {
#pragma unroll
      for (int c = 0; c < 9; ++c) W[(size_t)c * wstride + nd.row_off + r] = w[c];     // component-major: coalesced here and in the back substitution
    }
  };
  if (has0) finish_row(r0, sv0);
  for (int r = r0 + 256; r < m; r += 256) {
    double* srow = S + (size_t)rws[r] * ld + col;
    double sv[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) sv[c] = src.s_zero ? 0.0 : ld_s(srow + c);
    if (src.B) {
      const int oi = rnat[r];
      if (oi == -2) {
#pragma unroll
        for (int c = 0; c < 9; ++c) sv[c] -= src.gc[nb0 + c];
      } else if (oi >= 0) {
#pragma unroll
        for (int c = 0; c < 9; ++c) { const int oj = nb0 + c; sv[c] += src.B[(size_t)max(oi, oj) * src.ldB + min(oi, oj)]; }
      }
    }
    finish_row(r, sv);
  }
  if (tile == 0 && tid < 9) {              // column tid of L_bb^-1 (forward substitution against e_tid), for the back substitution
    double xcol[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      double v = (r == tid) ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < r; ++k) v -= L[r * 9 + k] * xcol[k];
      xcol[r] = v * linv[r];
    }
#pragma unroll
    for (int r = 0; r < 9; ++r) Lout[(size_t)ni * 81 + r * 9 + tid] = xcol[r];
  }
  __syncthreads();
  // S_NN -= W W^T.  The pairs whose COLUMN belongs to a sparse block (rows [0, ns): later (v, ba, bg) blocks come first in the ascending
  // row list) are what the next level reads; they go first, and a chained level signals its successor as soon as THEY are acknowledged —
  // the bulk (the dense corner's entries, four fifths at the top level) and its acknowledgement stay off the chain.
  int ns = 0;
  if (src.done_counter && src.strip_end > 0) {                  // (binary search: rws is ascending)
    int lo = 0, hi = m;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (rws[mid] < src.strip_end) lo = mid + 1; else hi = mid; }
    ns = lo;
  }
  auto pair_value = [&](const int r, const int c2) {
    const double* wr = Ws + r * 9;
    const double* wc = Ws + c2 * 9;
    double v = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) v += wr[c] * wc[c];
    return v;
  };
  auto pair_update = [&](const int r, const int c2) {
    const double v = pair_value(r, c2);
    if (v != 0.0) atomicAdd(&S[(size_t)rws[r] * ld + rws[c2]], -v);
  };
  if (ns > 0) {
    // RETURNING atomics: the value only comes back once the add has been performed where the next level will read it, so the barrier
    // below (which waits for the returns) really orders them ahead of the arrival.  With returnless adds the acknowledgement that
    // releases vmcnt came first often enough: 5 of 12 runs of the 8-keyframe / 20 000-landmark case had the next level read entries short of an update.
    double sink = 0.0;
    for (int q = tile * 256 + tid; q < ns * m; q += tiles * 256) {      // the m x ns rectangle, its r < c2 corner skipped
      const int r = q / ns, c2 = q - r * ns;
      if (r >= c2) {
        const double v = pair_value(r, c2);
        if (v != 0.0) sink += __hip_atomic_fetch_add(&S[(size_t)rws[r] * ld + rws[c2]], -v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (sink == -1.2345678901234567e301) atomicMax(fail, 50000);     // (never: keeps the returns alive)
  }
  if (stamp) stamp[5] = wall_clock64();
  if (src.done_counter) {
    __syncthreads();                       // every wave has its returns (the barrier drains vmcnt)
    if (tid == 0) {
      if (src.fenced) __hip_atomic_fetch_add((int*)src.done_counter, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      else __hip_atomic_fetch_add((int*)src.done_counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (stamp) stamp[6] = wall_clock64();
  const int m2 = m - ns, P = m2 * (m2 + 1) / 2;                          // the triangle over rows / columns [ns, m)
  for (int p = tile * 256 + tid; p < P; p += tiles * 256) {
    int r = (int)((sqrt(8.0 * p + 1.0) - 1.0) * 0.5);
    while ((r + 1) * (r + 2) / 2 <= p) ++r;
    while (r * (r + 1) / 2 > p) --r;
    const int c2 = p - r * (r + 1) / 2;
    pair_update(r + ns, c2 + ns);
  }
  if (stamp) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp[7] = wall_clock64(); }
}

template <bool SEL>
__device__ __forceinline__ void sp_ride(const int vb, const SpArgs& a) {
  if (vb >= a.nblocks) return;
  if (!SEL) { sp_eliminate_body(vb, a.nodes, a.first, a.tiles, a.rows, a.S, a.ld, a.W, a.wstride, a.Lout, a.fail, a.done, a.src); return; }
  SpSrc src = a.src;
  if (src.sel && *src.sel) { src.B = src.B1; src.gc = src.gc1; }      // (fused chain: the active accumulator set)
  sp_eliminate_body(vb, a.nodes, a.first, a.tiles, a.rows, a.S, a.ld, a.W, a.wstride, a.Lout, a.fail, a.done, src);
}
__global__ __launch_bounds__(256) void k_sp_eliminate(SpArgs a) { sp_ride<true>(blockIdx.x, a); }
__global__ __launch_bounds__(256) void k_sp_eliminate_b(const SpArgs* __restrict__ t) { sp_ride<false>(blockIdx.x, t[blockIdx.y]); }

// ------------------------------------------------------------------------------------------------ slab reduction / assembly
// Adds the TwoFrame slabs of a linearisation into B / gc (compact mode).  Workgroups are sorted by current keyframe: run(k) =
// workgroups [run_first[k], run_first[k+1]).  Every entry of B has ONE owner thread here (plain read-modify-write; the other factor
// types' atomic contributions were complete when the linearisation launch ended):
//   workgroups [0, n_kf)         keyframe k: B[k,k] (21) and g[k] (6) = sum of slabQ over run(k) (k as current keyframe)
//                                                                      + sum of slabP[.][k][0..27) over every later workgroup (k as first keyframe)
//   the rest                     one thread per (k2, k1 < k2, entry of the 6x6 cross block) = sum of slabP[.][k1][27..63) over run(k2)
template <bool SEL>
__device__ __forceinline__ void tf_reduce_body(const int bx0, const TfReduceArgs& A) {
  if (bx0 >= A.nblocks) {
    const int zw = (int)bx0 - A.nblocks;
    if (SEL && zw < A.zero_wgs) {
      if (acc_set(A.acc)) zero_list_share(A.stand0, zw, A.zero_wgs);
      else zero_list_share(A.stand1, zw, A.zero_wgs);
    }
    return;
  }
  if (A.done && *A.done) return;
  // (the riding level takes the FIRST workgroups: it is the longest piece of the launch, and in a batch the first workgroups of every
  // window are dispatched first — see the transposed table launches)
  if (bx0 < A.ride.nblocks) { sp_ride<SEL>(bx0, A.ride); return; }
  if (SEL && A.pending && !*A.pending) return;
  const bool s1 = acc_set_t<SEL>(A.acc) != 0;
  double* const Bs = s1 ? (double*)A.acc.B : (double*)A.B;
  double* const gcs = s1 ? (double*)A.acc.gc : (double*)A.gc;
  const int bx = bx0 - A.ride.nblocks;
  const int n_kf = A.n_kf;
  const int nchunk = (A.n_wg + 63) / 64;
  if (bx < n_kf * nchunk) {
    // keyframe k, chunk c of 64 workgroups: 8 groups of 32 lanes (lane v < 27 owns one value), 8 slab rows per thread, all requested at
    // once; the chunk's 27 sums go to B / gc with one atomic each (n_kf x nchunk x 27 per linearisation)
    __shared__ double part[8][32];
    const int k = bx / nchunk, c = bx - k * nchunk, v = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int r0 = A.run_first[k], r1 = A.run_first[k + 1];
    double acc = 0.0;
    if (v < 27) {
      // the eight slab values are requested together — the row (P or Q slab) chosen by address, the workgroup index clamped — and added in
      // order afterwards: as `if (wg >= r1) acc += P[..]; else if (wg >= r0) acc += Q[..]` every load sat in its own branch behind the
      // previous addition, eight dependent round trips per thread
      const double* slabP = A.slabP; const double* slabQ = A.slabQ;
      double t8[8]; bool keep[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int wg = 64 * c + g + 8 * u, wgc = min(wg, A.n_wg - 1);
        const bool useP = wgc >= r1;               // k as the blocks' first keyframe (later workgroups); else k as their current keyframe
        keep[u] = (wg < A.n_wg) & (wgc >= r0);
        const double* src = useP ? slabP + ((size_t)wgc * n_kf + k) * kSlabRow + v : slabQ + (size_t)wgc * kSlabQ + v;
        t8[u] = *src;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = keep[u] ? acc + t8[u] : acc;
    }
    part[g][v] = acc;
    __syncthreads();
    if (threadIdx.x < 27) {
      double t = 0.0;
#pragma unroll
      for (int q = 0; q < 8; ++q) t += part[q][threadIdx.x];
      if (t != 0.0) {
        if (threadIdx.x < 21) {
          int x = 0, rem = threadIdx.x;
          while (rem > x) { rem -= x + 1; ++x; }
          atomicAdd(&Bs[(size_t)(6 * k + x) * A.ld + 6 * k + rem], t);
        } else atomicAdd(&gcs[6 * k + threadIdx.x - 21], t);
      }
    }
    return;
  }
  const int e = (bx - n_kf * nchunk) * kT + threadIdx.x;
  const int npair = n_kf * (n_kf - 1) / 2;
  if (e >= npair * 36) return;
  const int pr = e / 36, el = e - 36 * pr;
  int k2 = (int)((1.0 + sqrt(1.0 + 8.0 * pr)) * 0.5);                 // pr = k2 (k2 - 1) / 2 + k1, k1 < k2
  while (k2 * (k2 - 1) / 2 > pr) --k2;
  while ((k2 + 1) * k2 / 2 <= pr) ++k2;
  const int k1 = pr - k2 * (k2 - 1) / 2;
  double acc = 0.0;
  {
    const double* slabP = A.slabP;
    const int w0 = A.run_first[k2], w1 = A.run_first[k2 + 1];
    for (int wg = w0; wg < w1; wg += 4) {            // four rows per round trip (index clamped), added in order
      double t4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) t4[u] = slabP[((size_t)min(wg + u, w1 - 1) * n_kf + k1) * kSlabRow + 27 + el];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = (wg + u < w1) ? acc + t4[u] : acc;
    }
  }
  if (acc != 0.0) {
    const int x = el / 6, y = el - 6 * x;                              // x: k2 tangent index, y: k1 tangent index
    Bs[(size_t)(6 * k2 + x) * A.ld + 6 * k1 + y] += acc;
  }
}
__global__ __launch_bounds__(kT) void k_tf_reduce(TfReduceArgs a) { tf_reduce_body<true>(blockIdx.x, a); }
__global__ __launch_bounds__(kT) void k_tf_reduce_b(const TfReduceArgs* __restrict__ t) { tf_reduce_body<false>(blockIdx.x, t[blockIdx.y]); }
// (transposed: blockIdx.x = window.  Workgroups are dispatched x-fastest, so the first workgroups of EVERY window — the riding / chained
// sparse levels, the ImuError factors — start together at the head of the launch instead of each window's behind the previous window's bulk)
__global__ __launch_bounds__(kT) void k_tf_reduce_bt(const TfReduceArgs* __restrict__ t) { tf_reduce_body<false>(blockIdx.y, t[blockIdx.x]); }

// One launch prepares the damped system of a step:
//   blocks [0, nS_blocks)      : S (lower, in ELIMINATION order: S row I holds unknown iperm[I]) = B (lower, natural order) + Dc on
//                                the diagonal; augmented row (iperm = -2) = -gc ; padding rows (iperm = -1) = identity
//   blocks [nS_blocks, ...)    : Cd = C + clamp(C)/radius ; E[l][dp] = gr[l] (the extra column that makes the SYRK also
//                                produce E^T Cd^-1 g_rho)
//   block 0 / thread 0         : resets the per-step scalars (candidate cost, model change, norms) and the Cholesky fail flag
template <bool SEL>
__device__ __forceinline__ void prepare_body(const unsigned bx0, const PrepArgs& A) {
  if (bx0 >= (unsigned)A.nblocks || (A.done && *A.done)) return;
  if (bx0 < (unsigned)A.ride.nblocks) { sp_ride<SEL>((int)bx0, A.ride); return; }      // (riders first: tf_reduce_body)
  const unsigned bx = bx0 - (unsigned)A.ride.nblocks;
  const bool s1 = acc_set_t<SEL>(A.acc) != 0;
  const int ld = A.ld, dpad = A.dpad; const int* __restrict__ iperm = A.iperm; const double* __restrict__ B = s1 ? (const double*)A.acc.B : (const double*)A.B;
  const double* __restrict__ gc = s1 ? (const double*)A.acc.gc : (const double*)A.gc;
  const double inv_radius = 1.0 / *A.radius;
  const int jf = *A.jac.frozen;
  double* __restrict__ S = A.S; const unsigned nS_blocks = A.nS_blocks; const int n_lm = A.n_lm, dp = A.dp, ldE = A.ldE;
  const double* __restrict__ C = s1 ? (const double*)A.acc.C : (const double*)A.C; const double* __restrict__ gr = s1 ? (const double*)A.acc.gr : (const double*)A.gr;
  double* __restrict__ Cd = A.Cd; double* __restrict__ E = s1 ? (double*)A.acc.E : (double*)A.E; double* __restrict__ scal = A.scal;
  const double* const slotB = (s1 && A.slotB) ? (const double*)A.acc.slotB : (const double*)A.slotB;
  if (bx == 0 && scal) reset_step_scalars(scal);
  if (bx >= nS_blocks) {
    if (slotB) {
      // atomic-free mode: C, g_rho of the landmark = its TwoCamera part (C, gr: atomics of the linearisation) + its slot records; the k1
      // columns of its E row = the sum of the records' first-keyframe parts.  8 lanes per landmark (lane j takes slots j, j + 8, ...: the
      // loads of a track are issued together instead of one dependent loop), DPP sum over the 8 lanes.  The totals go to separate arrays
      // so the pass can be repeated (lvf_problem_download_reduced).
      const int l = ((bx - nS_blocks) * kT + threadIdx.x) >> 3, j0 = threadIdx.x & 7;
      const bool live = l < n_lm;
      const int lc = live ? l : 0;
      const int k1 = A.kmin[lc], len = live ? max(0, A.kmax[lc] - k1) : 0;
      const double h0l = A.jac.h0[A.jl0 + lc];
      const double2* sb = reinterpret_cast<const double2*>(slotB + (size_t)A.eoff[lc] * 8);
      double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int j = j0; j < len; j += 8) {
        const double2 b0 = sb[4 * j], b1 = sb[4 * j + 1], b2 = sb[4 * j + 2], cg = sb[4 * j + 3];
        v[0] += cg.x; v[1] += cg.y; v[2] += b0.x; v[3] += b0.y; v[4] += b1.x; v[5] += b1.y; v[6] += b2.x; v[7] += b2.y;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) { v[q] = quad_sum(v[q]); v[q] += quad_perm<0x141>(v[q]); }      // sum over the aligned group of 8 lanes
      if (live && j0 == 0) {
        const double c = C[l] + v[0], g = gr[l] + v[1];
        A.Ct[l] = c; A.grt[l] = g;
        Cd[l] = c + lm_damping_fast_own(c, A.jac, A.jl0 + l, jf, h0l) * inv_radius;
        double* el = E + (size_t)l * ldE;
        el[dp] = g;
        if (len > 0) {
#pragma unroll
          for (int q = 0; q < 6; ++q) el[6 * k1 + q] = v[2 + q];
        }
      }
      return;
    }
    const int l = (bx - nS_blocks) * kT + threadIdx.x;
    if (l >= n_lm) return;
    const double c = C[l], h0l = A.jac.h0[A.jl0 + l];
    Cd[l] = c + lm_damping_fast_own(c, A.jac, A.jl0 + l, jf, h0l) * inv_radius;
    E[(size_t)l * ldE + dp] = gr[l];
    return;
  }
  // Only the LOWER triangle is assembled (nothing downstream reads an entry right of the diagonal as a value: the factorisations work
  // on lower tiles, and what they carry in the upper halves of diagonal tiles only ever feeds those same entries).  The triangle is
  // folded into a rectangle so that consecutive threads still write consecutive entries of a row: rectangle row q holds matrix row q
  // (columns 0..q) followed by matrix row ld-1-q (columns 0..ld-1-q), ld + 1 entries in all.
  const size_t e = (size_t)bx * kT + threadIdx.x;
  const int n0 = A.early ? A.off : 0, nn = ld - n0;                   // early form: the dense corner only
  const int half = (nn + 1) / 2;
  if (e >= (size_t)half * (nn + 1)) return;
  const int q = (int)(e / (nn + 1)), cc = (int)(e % (nn + 1));
  int I, J;
  if (cc <= q) { I = q; J = cc; }
  else { I = nn - 1 - q; J = cc - q - 1; if (I == q) return; }      // (odd size: the middle row is its own partner)
  I += n0; J += n0;
  const int oi = iperm[I], oj = iperm[J];
  double v = 0.0;
  if (oi >= 0) {
    if (oj >= 0 && J <= I) {
      const double h0d = I == J ? A.jac.h0[oi] : 0.0;
      v = B[(size_t)max(oi, oj) * dpad + min(oi, oj)];
      if (I == J) v += lm_damping_fast_own(v, A.jac, oi, jf, h0d) * inv_radius;
    }
  } else if (oi == -2) {
    v = (oj >= 0) ? -gc[oj] : (J == I ? 1e300 : 0.0);   // huge corner keeps the augmented matrix positive definite
  } else if (I == J) {
    v = 1.0;
  }
  if (!A.early) S[(size_t)I * ld + J] = v;
  else if (v != 0.0) atomicAdd(&S[(size_t)I * ld + J], v);
}
__global__ __launch_bounds__(kT) void k_prepare(PrepArgs a) { prepare_body<true>(blockIdx.x, a); }
__global__ __launch_bounds__(kT) void k_prepare_b(const PrepArgs* __restrict__ t) { prepare_body<false>(blockIdx.x, t[blockIdx.y]); }
__global__ __launch_bounds__(kT) void k_prepare_bt(const PrepArgs* __restrict__ t) { const PrepArgs a = t[blockIdx.x]; prepare_body<false>(blockIdx.y, a); }

// ------------------------------------------------------------------------------------------------ Schur reduce (MFMA f64)
// T = Ea^T diag(1/Cd) Ea with Ea = [E | g_rho] (n_lm x ldE).  One wave per (16x16 output tile, K-chunk); tiles on or
// below the diagonal only.  v_mfma_f64_16x16x4_f64: A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15],
// D: col = lane&15, row = (lane>>4) + 4*reg.   S[i][j] -= T[i][j] (i,j < dp);  S[d][i] += T[dp][i].
__global__ __launch_bounds__(64) void k_schur_syrk(int n_lm, int dp, int ldE, int ntile, const double* __restrict__ E,
                                                   const double* __restrict__ Cd, int d, int ldS, double* __restrict__ S) {
  // decode lower-triangular tile index
  int t = blockIdx.x, ti = 0;
  while (t >= ti + 1) { t -= ti + 1; ++ti; }
  const int tj = t;
  const int lane = threadIdx.x, lk = lane >> 4, lc = lane & 15;
  const int k_begin = blockIdx.y * kSchurChunk, k_end = min(n_lm, k_begin + kSchurChunk);
  double4_t acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = k_begin; k0 < k_end; k0 += 4) {
    const int l = k0 + lk;
    double a = 0.0, b = 0.0;
    if (l < k_end) {
      const double* row = E + (size_t)l * ldE;
      a = row[ti * 16 + lc] / Cd[l];
      b = row[tj * 16 + lc];
    }
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int gi = ti * 16 + lk + 4 * r, gj = tj * 16 + lc;
    const double v = acc[r];
    if (v == 0.0) continue;
    if (gi < dp && gj < dp) { if (gj <= gi) atomicAdd(&S[(size_t)gi * ldS + gj], -v); }
    else if (gi == dp && gj < dp) atomicAdd(&S[(size_t)d * ldS + gj], v);
  }
}

// LDS-staged variant (used whenever ldE <= 320, i.e. up to 53 keyframes; larger windows fall back to k_schur_syrk): workgroup = (tile group g of kSchurGroups, K slice).  The slice's rows
// of Ea are streamed through LDS in 16-row chunks with fully coalesced loads (the next chunk is prefetched into registers while
// the current one feeds the matrix cores); every wave keeps up to kSchurTilesPerWave 16x16 accumulators in registers across
// the whole slice and the workgroup touches S once at the end.  Versus one wave per (tile, 512-row chunk) with strided 8-byte
// global operand loads: the same MFMA count, 1/8 of the atomics, and E is read once per tile group instead of once per tile.
__global__ __launch_bounds__(256) void k_schur_lds(int n_lm, int dp, int ldE, int ntile, int rows_per_slice, const double* __restrict__ E,
                                                   const double* __restrict__ Cd, int d, int ldS, double* __restrict__ S) {
  extern __shared__ double sh[];          // Es[kSchurRows][ldE] | icd[kSchurRows]
  double* Es = sh;
  double* icd = sh + kSchurRows * ldE;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, lk = lane >> 4, lc = lane & 15;
  const int g = blockIdx.x, slice = blockIdx.y;
  const int k_begin = slice * rows_per_slice, k_end = min(n_lm, k_begin + rows_per_slice);
  // this wave's tiles: t = g + kSchurGroups * (w + 4 * s), s = 0..; decode (ti, tj) of the lower-triangular enumeration
  int ti[kSchurTilesPerWave], tj[kSchurTilesPerWave], nt = 0;
#pragma unroll
  for (int s_ = 0; s_ < kSchurTilesPerWave; ++s_) {
    const int t = g + kSchurGroups * (w + 4 * s_);
    ti[s_] = 0; tj[s_] = 0;
    if (t < ntile) {
      int a = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
      while ((a + 1) * (a + 2) / 2 <= t) ++a;
      while (a * (a + 1) / 2 > t) --a;
      ti[s_] = a; tj[s_] = t - a * (a + 1) / 2;
      nt = s_ + 1;
    }
  }
  double4_t acc[kSchurTilesPerWave];
#pragma unroll
  for (int s_ = 0; s_ < kSchurTilesPerWave; ++s_) acc[s_] = double4_t{0.0, 0.0, 0.0, 0.0};
  const int per_row = ldE;                 // doubles per staged row
  const int total = kSchurRows * per_row;  // elements per chunk
  constexpr int kPf = 20;                  // prefetch registers per thread: 256 * 20 >= 16 * 304 (ldE <= 320 on this path; larger ldE loops)
  double pf[kPf];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int u = 0; u < kPf; ++u) {
      const int e = tid + 256 * u;
      double v = 0.0;
      if (e < total) { const int rr = e / per_row, cc = e - rr * per_row; if (k0 + rr < k_end) v = E[(size_t)(k0 + rr) * ldE + cc]; }
      pf[u] = v;
    }
  };
  auto fetch_tail = [&](int k0) {         // elements beyond 256 * kPf (only when ldE > 320): straight to LDS
    for (int e = tid + 256 * kPf; e < total; e += 256) {
      const int rr = e / per_row, cc = e - rr * per_row;
      Es[e] = (k0 + rr < k_end) ? E[(size_t)(k0 + rr) * ldE + cc] : 0.0;
    }
  };
  if (k_begin < k_end) fetch(k_begin);
  for (int k0 = k_begin; k0 < k_end; k0 += kSchurRows) {
    __syncthreads();                       // the previous chunk has been consumed
#pragma unroll
    for (int u = 0; u < kPf; ++u) { const int e = tid + 256 * u; if (e < total) Es[e] = pf[u]; }
    fetch_tail(k0);
    if (tid < kSchurRows) icd[tid] = (k0 + tid < k_end) ? 1.0 / Cd[k0 + tid] : 0.0;
    __syncthreads();
    if (k0 + kSchurRows < k_end) fetch(k0 + kSchurRows);   // in flight while the matrix cores work
#pragma unroll
    for (int kk = 0; kk < kSchurRows; kk += 4) {
      const double* row = Es + (kk + lk) * per_row;
      const double wgt = icd[kk + lk];
#pragma unroll
      for (int s_ = 0; s_ < kSchurTilesPerWave; ++s_)
        if (s_ < nt) acc[s_] = __builtin_amdgcn_mfma_f64_16x16x4f64(row[16 * ti[s_] + lc] * wgt, row[16 * tj[s_] + lc], acc[s_], 0, 0, 0);
    }
  }
#pragma unroll
  for (int s_ = 0; s_ < kSchurTilesPerWave; ++s_) {
    if (s_ >= nt) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gi = ti[s_] * 16 + lk + 4 * r, gj = tj[s_] * 16 + lc;
      const double v = acc[s_][r];
      if (v == 0.0) continue;
      if (gi < dp && gj < dp) { if (gj <= gi) atomicAdd(&S[(size_t)gi * ldS + gj], -v); }
      else if (gi == dp && gj < dp) atomicAdd(&S[(size_t)d * ldS + gj], v);
    }
  }
}
// ---- band-limited variant.  A landmark's row of E is non-zero only at the keyframes that observe it, a contiguous track
// [kmin_l, kmax_l] of the window.  Landmarks are ordered by (track-length class, kmin) once per problem (k_lm_range + k_lm_sort),
// so a slice of kBandRows consecutive landmarks touches a narrow BAND of 16-column tiles [t0, t1]: the workgroup stages only
// those columns (plus the tile holding the g_rho column) and only forms the band's lower-triangular tiles.  At configs[3]
// that is ~1/5 of the MFMAs and ~1/30 of the E bytes of the dense SYRK.  Correctness never depends on the ordering: the
// band of each slice is computed from the actual kmin/kmax of its rows.
__global__ __launch_bounds__(kT) void k_lm_range(int n, const int* __restrict__ lm, const int* __restrict__ k1, const int* __restrict__ k2,
                                                 int* __restrict__ kmin, int* __restrict__ kmax) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const int l = lm[i], a = min(k1[i], k2[i]), b = max(k1[i], k2[i]);
  atomicMin(&kmin[l], a); atomicMax(&kmax[l], b);
}
__device__ __forceinline__ int lm_sort_key(int kmin, int kmax, int n_kf) {
  // (branch-free on purpose: with `if (kmax < 0) return ..` in front, the compiler sinks the caller's kmin load into the branch behind the
  // kmax load's wait — two dependent round trips per landmark instead of one)
  const int len = kmax - kmin + 1;
  const int cls = (len > 8) + (len > 16) + (len > 32);
  const int none = kmax >> 31;                          // all ones: no pose-dependent block — nothing to eliminate, ordered last
  return (none & (4 * n_kf)) | (~none & (cls * n_kf + kmin));
}
// counting sort by key, one workgroup (n_lm is ~1e4; 4 n_kf + 1 buckets in LDS)
// (per-wave copies of the histogram — 16x fewer lanes per address — measured SLOWER, 15.7 vs 13.6 us: the two passes are bound by their
// dependent load -> LDS atomic round trips, not by address conflicts)
__device__ __forceinline__ void lm_sort_body(int n_lm, int n_kf, const int* __restrict__ kmin, const int* __restrict__ kmax,
                                             int* __restrict__ order, int* __restrict__ n_active) {
  extern __shared__ int bucket[];
  const int nb = 4 * n_kf + 1;
  for (int b = threadIdx.x; b < nb; b += 1024) bucket[b] = 0;
  __syncthreads();
  // (16 landmarks per thread and pass, their tracks requested together and the keys kept for the second sweep: as `for (l ..) atomicAdd(&bucket[
  // key(kmin[l], kmax[l])], 1)` every iteration waited for its own two loads before its LDS atomic — twice ten dependent round trips at 10 k landmarks)
  constexpr int kG = 16;
  for (int sb = 0; sb < n_lm; sb += kG * 1024) {
    int key[kG];
#pragma unroll
    for (int g = 0; g < kG; ++g) { const int lc = min(sb + g * 1024 + (int)threadIdx.x, n_lm - 1); key[g] = lm_sort_key(kmin[lc], kmax[lc], n_kf); }
#pragma unroll
    for (int g = 0; g < kG; ++g) if (sb + g * 1024 + (int)threadIdx.x < n_lm) atomicAdd(&bucket[key[g]], 1);
  }
  __syncthreads();
  if (nb <= 1024) {                         // exclusive scan of the bucket counts: 16 wave scans + 16 wave totals
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = tid < nb ? bucket[tid] : 0;
    const int incl = wave_incl_scan(c);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    if (tid < nb) bucket[tid] = base + incl - c;
    if (tid == nb - 1) *n_active = base + incl - c;
  } else if (threadIdx.x == 0) {
    int run = 0;
    for (int b = 0; b < nb; ++b) { const int c = bucket[b]; bucket[b] = run; run += c; }
    *n_active = bucket[nb - 1];
  }
  __syncthreads();
  for (int sb = 0; sb < n_lm; sb += kG * 1024) {
    int key[kG];
#pragma unroll
    for (int g = 0; g < kG; ++g) { const int lc = min(sb + g * 1024 + (int)threadIdx.x, n_lm - 1); key[g] = lm_sort_key(kmin[lc], kmax[lc], n_kf); }
#pragma unroll
    for (int g = 0; g < kG; ++g) { const int l = sb + g * 1024 + (int)threadIdx.x; if (l < n_lm) order[atomicAdd(&bucket[key[g]], 1)] = l; }
  }
}
__global__ __launch_bounds__(1024) void k_lm_sort(int n_lm, int n_kf, const int* __restrict__ kmin, const int* __restrict__ kmax,
                                                  int* __restrict__ order, int* __restrict__ n_active) {
  lm_sort_body(n_lm, n_kf, kmin, kmax, order, n_active);
}

// ---- compact landmark layout, built once per problem_configure
// eoff[l] = first slot of landmark l, len_l = kmax_l - kmin_l slots (one per keyframe after the first); *n_slots = their total
__device__ __forceinline__ void lm_offsets_body(int n_lm, const int* __restrict__ kmin, const int* __restrict__ kmax, int* __restrict__ eoff,
                                                int* __restrict__ n_slots) {
  // 16 k landmarks per pass: every thread requests its 16 (kmin, kmax) pairs up front (a load inside the per-1024 loop was waited for
  // before the next was issued: 10 dependent round trips at 10 k landmarks), scans run inside waves, two workgroup barriers per pass
  constexpr int kG = 16;
  __shared__ int s_cnt[kG * 16];                    // [chunk][wave] totals, then their exclusive prefix
  __shared__ int s_total;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int total = 0;
  for (int sb = 0; sb < n_lm; sb += kG * 1024) {
    int c[kG], ex[kG];
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      const int l = sb + g * 1024 + tid, lc = min(l, n_lm - 1);
      const int lo = kmin[lc], hi = kmax[lc];
      c[g] = max(0, hi - lo) & -(int)((l < n_lm) & (hi >= 0));      // (branch-free: behind `l < n_lm && hi >= 0 ? .. : 0` the kmin load was sunk into a branch behind the kmax load's wait, 32 dependent round trips)
    }
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      const int incl = wave_incl_scan(c[g]);
      ex[g] = incl - c[g];
      if (lane == 63) s_cnt[g * 16 + wave] = incl;
    }
    __syncthreads();
    if (wave == 0) {                                 // exclusive scan of the 256 totals (chunk-major = ascending landmark order)
      int carry = 0;
#pragma unroll
      for (int base = 0; base < kG * 16; base += 64) {
        const int v = s_cnt[base + lane];
        const int inc = wave_incl_scan(v);
        s_cnt[base + lane] = carry + inc - v;
        carry += __shfl(inc, 63);
      }
      if (lane == 0) s_total = carry;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      const int l = sb + g * 1024 + tid;
      if (l < n_lm) eoff[l] = total + s_cnt[g * 16 + wave] + ex[g];
    }
    total += s_total;
    __syncthreads();
  }
  if (tid == 0) *n_slots = total;
}
// the counting sort and the slot offsets are two one-workgroup chains over the same (kmin, kmax) with nothing in common but their inputs:
// ONE launch of two workgroups runs them side by side (a persistent window reconfigures every tick: 14 us + 9 us + a launch gap became 14 us)
__global__ __launch_bounds__(1024) void k_lm_sort_offsets(int n_lm, int n_kf, const int* __restrict__ kmin, const int* __restrict__ kmax, int* __restrict__ order,
                                                          int* __restrict__ n_active, int* __restrict__ eoff, int* __restrict__ n_slots) {
  if (blockIdx.x == 0) lm_sort_body(n_lm, n_kf, kmin, kmax, order, n_active);
  else lm_offsets_body(n_lm, kmin, kmax, eoff, n_slots);
}
// Two jobs in one launch: workgroups [0, g_slots) give every TwoFrame block its slot in its landmark's track (eoff[l] + keyframes after the
// first), the rest clear the slot records — slots of keyframes that do not observe their landmark (gaps in a track) are never written by
// the linearisation, so they are cleared once here
__global__ __launch_bounds__(kT) void k_tf_slots_zero(int n, int g_slots, const int* __restrict__ lm, const int* __restrict__ k2, const int* __restrict__ kmin,
                                                      const int* __restrict__ eoff, int* __restrict__ slot, const int* __restrict__ n_slots, double* __restrict__ slotB) {
  if ((int)blockIdx.x < g_slots) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const int l = lm[i];
    slot[i] = eoff[l] + (k2[i] - kmin[l] - 1);
    return;
  }
  const size_t nz = (size_t)*n_slots * 4;     // double2 elements
  double2* b = reinterpret_cast<double2*>(slotB);
  const size_t gz = gridDim.x - g_slots;
  for (size_t i = (size_t)(blockIdx.x - g_slots) * kT + threadIdx.x; i < nz; i += gz * kT) b[i] = make_double2(0.0, 0.0);
}
// sorted copies of the TwoFrame block arrays: block i of the copy = block perm[i] of the batch
__global__ __launch_bounds__(kT) void k_tf_gather(int n, const int* __restrict__ perm, const double2* __restrict__ fo, const double2* __restrict__ ob,
                                                   const int* __restrict__ lm, const int* __restrict__ k1, const int* __restrict__ k2,
                                                   double2* __restrict__ fo_s, double2* __restrict__ ob_s, int* __restrict__ lm_s, int* __restrict__ k1_s, int* __restrict__ k2_s) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const int j = perm[i];
  fo_s[i] = fo[j]; ob_s[i] = ob[j]; lm_s[i] = lm[j]; k1_s[i] = k1[j]; k2_s[i] = k2[j];
}
// Work list of the band Schur complement: one item per (slice, tile group) that has tiles to form.  The 2-D grid slices x groups is sized
// for the widest possible band, but most slices (short tracks) need one group: three quarters of its workgroups had nothing to do and
// their dispatch — each needs its LDS slice — was most of the launch's span.  Built once per problem_configure (the bands are fixed).
__global__ __launch_bounds__(64) void k_band_work(int rows, int dp, const int* __restrict__ n_active_p, const int* __restrict__ order,
                                                  const int* __restrict__ kmin, const int* __restrict__ kmax, int4* __restrict__ work, int* __restrict__ n_work) {
  const int n_active = *n_active_p, lane = threadIdx.x;
  const int k_begin = blockIdx.x * rows, k_end = min(n_active, k_begin + rows);
  if (k_begin >= k_end) return;
  int lo = 0x7fffffff, hi = -1;
  for (int r = k_begin + lane; r < k_end; r += 64) { const int l = order[r]; lo = min(lo, kmin[l]); hi = max(hi, kmax[l]); }
  for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
  if (lane == 0) {
    const int t0 = (6 * lo) >> 4, t1 = (6 * hi + 5) >> 4, tl = dp >> 4, nbt = t1 - t0 + 1;
    const int ntiles = nbt * (nbt + 1) / 2 + (tl > t1 ? nbt : 0);
    const int groups = (ntiles + kBandTilesPerGroup - 1) / kBandTilesPerGroup;
    const int base = atomicAdd(n_work, groups);
    for (int g = 0; g < groups; ++g) work[base + g] = make_int4((int)blockIdx.x, g, lo | (hi << 16), k_end);
  }
}

__device__ __forceinline__ void schur_band_body(const int bx, const int by, int dp, int ldE, const double* __restrict__ E,
                                                const double* __restrict__ Cd, const int* __restrict__ order, const int* __restrict__ n_active_p,
                                                const int* __restrict__ kmin, const int* __restrict__ kmax, int d, int ldS,
                                                double* __restrict__ S, unsigned long long* dbg = nullptr, const int rows = kBandRows,
                                                const int4* __restrict__ item = nullptr) {
  extern __shared__ double sh[];          // Es[kSchurRows][ldl] | icd[kSchurRows] | rowid (int)[kBandRows]
  auto mark = [&](int k) { if (dbg && threadIdx.x == 0) dbg[k] = wall_clock64(); };   // LVF_SCHUR_TIMING=1: phase stamps of this workgroup
  mark(0);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, lk = lane >> 4, lc = lane & 15;
  // the slice's extent and band: from the work item when there is one (k_band_work computed them once per configure: three dependent
  // global round trips — n_active, order[], kmin/kmax[] — off the front of every workgroup), else every wave reduces them for itself
  const int k_begin = bx * rows;
  int k_end, lo = 0x7fffffff, hi = -1;
  if (item) { const int4 it = *item; k_end = it.w; lo = it.z & 0xffff; hi = it.z >> 16; }
  else {
    k_end = min(*n_active_p, k_begin + rows);
    if (k_begin >= k_end) return;
    for (int r = k_begin + lane; r < k_end; r += 64) { const int l = order[r]; lo = min(lo, kmin[l]); hi = max(hi, kmax[l]); }
    for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
  }
  const int t0 = (6 * lo) >> 4, t1 = (6 * hi + 5) >> 4, tl = dp >> 4;
  const int nbt = t1 - t0 + 1, tri = nbt * (nbt + 1) / 2;
  const bool extra = tl > t1;                                  // the g_rho column's tile lies outside the band
  const int ntiles = tri + (extra ? nbt : 0);
  const int tbase = by * kBandTilesPerGroup;
  if (tbase >= ntiles) return;
  const int ldl = 16 * (nbt + (extra ? 1 : 0));                // staged doubles per row
  double* Es = sh;
  double* icd = sh + kSchurRows * (ldE + 16);
  int* rowid = reinterpret_cast<int*>(icd + kSchurRows);
  for (int r = tid; r < rows; r += 256) rowid[r] = (k_begin + r < k_end) ? order[k_begin + r] : -1;
  // this wave's tiles: t = tbase + w + 4 s; local tile columns (a = row tile, b = column tile), extra row tile = index nbt
  int ta[kBandTilesPerWave], tb[kBandTilesPerWave], nt = 0;
#pragma unroll
  for (int s_ = 0; s_ < kBandTilesPerWave; ++s_) {
    const int t = tbase + w + 4 * s_;
    ta[s_] = 0; tb[s_] = 0;
    if (t < ntiles) {
      if (t < tri) {
        int a = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
        while ((a + 1) * (a + 2) / 2 <= t) ++a;
        while (a * (a + 1) / 2 > t) --a;
        ta[s_] = a; tb[s_] = t - a * (a + 1) / 2;
      } else { ta[s_] = nbt; tb[s_] = t - tri; }
      nt = s_ + 1;
    }
  }
  double4_t acc[kBandTilesPerWave];
#pragma unroll
  for (int s_ = 0; s_ < kBandTilesPerWave; ++s_) acc[s_] = double4_t{0.0, 0.0, 0.0, 0.0};
  // staging: thread (row fr = tid >> 4, column fc = tid & 15) carries column fc of every staged 16-column tile of its row:
  // no index arithmetic beyond one add per tile, 128-byte runs per 16 lanes
  constexpr int kPf = 20;                  // tiles prefetched in registers (ldl <= 320); wider bands finish through fetch_tail
  double pf[kPf];
  double pf_cd = 1.0;
  const int fr = tid >> 4, fc = tid & 15, nst = ldl >> 4;
  __syncthreads();                         // rowid
  auto fetch = [&](int k0) {
    const int l = rowid[k0 - k_begin + fr];
    const double* src = E + (size_t)max(l, 0) * ldE + fc;
    if (fc == 0) pf_cd = (l >= 0) ? Cd[l] : 1.0;
#pragma unroll
    for (int u = 0; u < kPf; ++u) {
      double v = 0.0;
      if (u < nst && l >= 0) v = src[16 * (u < nbt ? t0 + u : tl)];
      pf[u] = v;
    }
  };
  auto fetch_tail = [&](int k0) {
    const int l = rowid[k0 - k_begin + fr];
    for (int u = kPf; u < nst; ++u) Es[fr * ldl + 16 * u + fc] = (l >= 0) ? E[(size_t)l * ldE + 16 * (u < nbt ? t0 + u : tl) + fc] : 0.0;
  };
  fetch(k_begin);
  mark(1);
  for (int k0 = k_begin; k0 < k_end; k0 += kSchurRows) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kPf; ++u) if (u < nst) Es[fr * ldl + 16 * u + fc] = pf[u];
    fetch_tail(k0);
    if (fc == 0) icd[fr] = (rowid[k0 - k_begin + fr] >= 0) ? 1.0 / pf_cd : 0.0;
    __syncthreads();
    if (k0 + kSchurRows < k_end) fetch(k0 + kSchurRows);
#pragma unroll
    for (int kk = 0; kk < kSchurRows; kk += 4) {
      const double* row = Es + (kk + lk) * ldl;
      const double wgt = icd[kk + lk];
#pragma unroll
      for (int s_ = 0; s_ < kBandTilesPerWave; ++s_)
        if (s_ < nt) acc[s_] = __builtin_amdgcn_mfma_f64_16x16x4f64(row[16 * ta[s_] + lc] * wgt, row[16 * tb[s_] + lc], acc[s_], 0, 0, 0);
    }
  }
  mark(2);
#pragma unroll
  for (int s_ = 0; s_ < kBandTilesPerWave; ++s_) {
    if (s_ >= nt) continue;
    const int gti = ta[s_] < nbt ? t0 + ta[s_] : tl, gtj = t0 + tb[s_];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gi = gti * 16 + lk + 4 * r, gj = gtj * 16 + lc;
      const double v = acc[s_][r];
      if (v == 0.0) continue;
      if (gi < dp && gj < dp) { if (gj <= gi) atomicAdd(&S[(size_t)gi * ldS + gj], -v); }
      else if (gi == dp && gj < dp) atomicAdd(&S[(size_t)d * ldS + gj], v);
    }
  }
  mark(3);
}

__global__ __launch_bounds__(256) void k_schur_band(int dp, int ldE, const double* __restrict__ E, const double* __restrict__ Cd,
                                                    const int* __restrict__ order, const int* __restrict__ n_active_p,
                                                    const int* __restrict__ kmin, const int* __restrict__ kmax, int d, int ldS,
                                                    double* __restrict__ S) {
  schur_band_body(blockIdx.x, blockIdx.y, dp, ldE, E, Cd, order, n_active_p, kmin, kmax, d, ldS, S);
}

// The band-limited Schur complement and the FIRST sparse level in one launch: both only ADD (atomically) into entries of S the other
// does not read — the Schur complement touches the pose corner and the pose part of the rhs row, level 0 reads its own (v,ba,bg)
// columns — so they are independent; later levels depend on level 0 and stay launches of their own.
template <bool SEL>
__device__ __forceinline__ void schur_sp0_body(const int b, const SchurSp0Args& A) {
  if (b >= A.nblocks) return;
  if (A.work) {
    const int n_a = A.sp.nblocks, n_b = A.sp_b.nblocks, n_c = A.sp_c.nblocks, n_sp = n_a + n_b + n_c;
    if (b < n_a) sp_ride<SEL>(b, A.sp);
    else if (b < n_a + n_b) sp_ride<SEL>(b - n_a, A.sp_b);
    else if (b < n_sp) sp_ride<SEL>(b - n_a - n_b, A.sp_c);
    else {
      const int dv = done_flag_issue(A.done);
      const int set = acc_set_t<SEL>(A.acc);
      const int4* item = A.work + (b - n_sp);
      const int4 it = *item;
      if (dv) return;
      schur_band_body(it.x, it.y, A.dp, A.ldE, set ? (const double*)A.acc.E : (const double*)A.E, A.Cd, A.order, A.n_active, A.kmin, A.kmax, A.d_local, A.ldS, A.S_pose, A.dbg ? A.dbg + (size_t)(b - n_sp) * 8 : nullptr, A.rows, item);
    }
    return;
  }
  if (A.done && *A.done) return;
  const int ns = A.n_slices * A.n_groups;
  if (b < ns) schur_band_body(b % A.n_slices, b / A.n_slices, A.dp, A.ldE, acc_set_t<SEL>(A.acc) ? (const double*)A.acc.E : (const double*)A.E, A.Cd, A.order, A.n_active, A.kmin, A.kmax, A.d_local, A.ldS, A.S_pose, A.dbg ? A.dbg + (size_t)b * 8 : nullptr, A.rows);
  else sp_ride<SEL>(b - ns, A.sp);
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_schur_sp0(SchurSp0Args a) { schur_sp0_body<true>(blockIdx.x, a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_schur_sp0_b(const SchurSp0Args* __restrict__ t) { schur_sp0_body<false>(blockIdx.x, t[blockIdx.y]); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_schur_sp0_bt(const SchurSp0Args* __restrict__ t) { schur_sp0_body<false>(blockIdx.y, t[blockIdx.x]); }

}  // namespace lvf
