// solver_plan.hip — what is decided once per problem_configure: the elimination plan of the (v, ba, bg) blocks (host) and the problem's
// buffers, TwoFrame work list, landmark tracks and compact layout (host + the layout kernels of solver_assemble.hip).
#include <algorithm>
#include <chrono>
#include <cstdlib>

#include "solver_host.hpp"

namespace lvf {

// Elimination plan (host, <= a few hundred nodes): which (v, ba, bg) blocks are factorised sparsely, in which level, with which
// neighbour rows; the S row of every unknown.  Rebuilt only when (n_kf, IMU index pairs) change.  LVF_SPARSE_VB=0 keeps every
// block in the dense corner (the round-1 layout, poses last) for A/B measurements.
//
// A keyframe of the problem's dense prior (lvf_problem_set_dense_prior) is never CHOSEN for sparse elimination: the prior couples its
// (v, ba, bg) block to its own pose, to the other keyframes of the prior and to their poses, none of which the ImuError adjacency knows, and
// its terms reach B only after the early levels have formed their columns.  Kept in the dense corner, the block is assembled by k_prepare,
// which runs behind the prior's launch and reads all of B.  It is still a neighbour row of the blocks that are eliminated, and still
// blocked by them, exactly as today; a problem without such a prior builds the key and the plan it always built.
static int build_elimination_plan(lvf_problem* p) {
  const int n = p->n_kf;
  std::vector<int32_t> key;
  key.push_back(n);
  const lvf_batch* imu = p->imu;
  const bool have_idx = imu && imu->n > 0 && (int)imu->host_kf1.size() == imu->n && (int)imu->host_kf2.size() == imu->n;
  if (imu && imu->n > 0) {
    key.push_back(have_idx ? 1 : 0);
    if (have_idx) { key.insert(key.end(), imu->host_kf1.begin(), imu->host_kf1.end()); key.insert(key.end(), imu->host_kf2.begin(), imu->host_kf2.end()); }
  }
  std::vector<char> pinned(n, 0);
  if (p->dprior) {
    std::vector<int32_t> kfs(p->dprior->kf_h);
    std::sort(kfs.begin(), kfs.end());
    key.push_back(INT32_MIN);                         // (no keyframe count or index is negative: the marker cannot be part of a key without a prior)
    key.insert(key.end(), kfs.begin(), kfs.end());
    for (int32_t k : kfs) if (k >= 0 && k < n) pinned[k] = 1;
  }
  if (key == p->plan_key && p->ld > 0) return LVF_OK;
  std::vector<std::vector<char>> va(n, std::vector<char>(n, 0)), pa(n, std::vector<char>(n, 0));
  bool sparse = solver_env().sparse_vb && (!imu || imu->n == 0 || have_idx);
  if (have_idx)
    for (int f = 0; f < imu->n; ++f) {
      const int i = imu->host_kf1[f], j = imu->host_kf2[f];
      if (i < 0 || j < 0 || i >= n || j >= n || i == j) continue;
      va[i][j] = va[j][i] = 1;
      pa[i][i] = pa[i][j] = pa[j][i] = pa[j][j] = 1;
    }
  struct NodeInfo { int kf; std::vector<int> vb, pose; };
  std::vector<NodeInfo> nodes;
  std::vector<char> alive(n, 1);
  SpLevels lv{};
  // How many levels to eliminate sparsely.  Whatever is left rides in the dense corner, which is factorised in 64-column block steps:
  // a level beyond the first (level 0 rides in the Schur launch) costs a launch (~8.5 us), a block step ~18 us.  A dry run of the greedy
  // level construction gives the number of blocks left after each level; the cut-off minimises 8.5 (levels - 1) + 18 block steps (measured launch costs, us).
  // (At 50 keyframes: 5 levels and one block in the corner's padding instead of 6 levels; at 5: level 0 only.)
  int max_levels = kSpMaxLevels;
  if (sparse) {
    std::vector<std::vector<char>> va2 = va;
    std::vector<char> alive2(n, 1);
    std::vector<int> left_after;                      // blocks left after level l
    for (int l = 0; l < kSpMaxLevels; ++l) {
      std::vector<char> blocked(n, 0);
      std::vector<int> chosen;
      for (int k = 0; k < n; ++k) {
        if (!alive2[k] || blocked[k] || pinned[k]) continue;
        chosen.push_back(k);
        for (int u = 0; u < n; ++u) if (va2[k][u]) blocked[u] = 1;
      }
      if (chosen.empty()) break;
      for (int b : chosen) {
        std::vector<int> nb_;
        for (int u = 0; u < n; ++u) if (va2[b][u] && alive2[u]) nb_.push_back(u);
        for (int u : nb_) { for (int w : nb_) if (w != u) va2[u][w] = 1; va2[u][b] = 0; }
        alive2[b] = 0;
      }
      int left = 0;
      for (int k = 0; k < n; ++k) left += alive2[k] ? 1 : 0;
      left_after.push_back(left);
    }
    double best = 1e300;
    for (size_t l = 0; l < left_after.size(); ++l) {
      const int steps = (9 * left_after[l] + p->dp + 1 + 63) / 64;
      const double cost = 8.5 * (double)l + 18.0 * steps;
      if (cost < best - 1e-9) { best = cost; max_levels = (int)l + 1; }
    }
    const int force_levels = solver_env().force_levels;      // experiment
    if (force_levels > 0) max_levels = std::min((int)left_after.size(), force_levels);
  }
  while (sparse && lv.n < std::min(max_levels, kSpMaxLevels)) {
    std::vector<char> blocked(n, 0);
    std::vector<int> chosen;
    for (int k = 0; k < n; ++k) {
      if (!alive[k] || blocked[k] || pinned[k]) continue;
      int m = 1;
      for (int u = 0; u < n; ++u) m += 9 * (va[k][u] && alive[u]) + 6 * pa[k][u];
      if (m > kSpMaxRows) continue;
      chosen.push_back(k);
      for (int u = 0; u < n; ++u) if (va[k][u]) blocked[u] = 1;
    }
    if (chosen.empty()) break;
    lv.first[lv.n] = (int)nodes.size(); lv.count[lv.n] = (int)chosen.size(); ++lv.n;
    for (int b : chosen) {
      NodeInfo ni; ni.kf = b;
      for (int u = 0; u < n; ++u) { if (va[b][u] && alive[u]) ni.vb.push_back(u); if (pa[b][u]) ni.pose.push_back(u); }
      nodes.push_back(std::move(ni));
    }
    for (size_t ci = 0; ci < chosen.size(); ++ci) {   // fill-in among the neighbours of an eliminated block
      const int b = chosen[ci];
      const NodeInfo& ni = nodes[lv.first[lv.n - 1] + (int)ci];
      for (int u : ni.vb) {
        for (int w : ni.vb) if (w != u) va[u][w] = 1;
        for (int k : ni.pose) pa[u][k] = 1;
        va[u][b] = 0;
      }
      alive[b] = 0;
    }
  }
  // S rows
  const int ns = (int)nodes.size();
  std::vector<int> vbcol(n, -1);
  for (int s_ = 0; s_ < ns; ++s_) vbcol[nodes[s_].kf] = 9 * s_;
  p->off = (9 * ns + 1) & ~1;
  int ndv = 0;
  for (int k = 0; k < n; ++k) if (alive[k]) vbcol[k] = p->off + 9 * ndv++;
  p->off_pose = p->off + 9 * ndv;
  p->ndense = 9 * ndv + p->dp;
  p->aug = p->off + p->ndense;
  p->nb = (p->ndense + 1 + 63) / 64;
  p->ld = p->off + 64 * p->nb;
  p->perm_h.assign(p->d, 0);
  std::vector<int> iperm(p->ld, -1);
  for (int i = 0; i < p->dp; ++i) p->perm_h[i] = p->off_pose + i;
  for (int k = 0; k < n; ++k) for (int c = 0; c < 9; ++c) p->perm_h[p->dp + 9 * k + c] = vbcol[k] + c;
  for (int i = 0; i < p->d; ++i) iperm[p->perm_h[i]] = i;
  iperm[p->aug] = -2;
  // device tables
  std::vector<SpNode> dn(ns);
  std::vector<int> rows, owner, rows_nat;
  p->sp_tiles.assign(lv.n, 1); p->sp_shmem.assign(lv.n, 0); p->sp_item0.assign(lv.n, 0); p->sp_items.assign(lv.n, 0);
  for (int l = 0; l < lv.n; ++l) {
    int mmax = 0;
    for (int s_ = lv.first[l]; s_ < lv.first[l] + lv.count[l]; ++s_) {
      const NodeInfo& ni = nodes[s_];
      dn[s_].col = 9 * s_; dn[s_].row_off = (int)rows.size(); dn[s_].id = ni.kf;
      std::vector<int> r;
      for (int u : ni.vb) for (int c = 0; c < 9; ++c) r.push_back(vbcol[u] + c);
      for (int k : ni.pose) for (int c = 0; c < 6; ++c) r.push_back(p->off_pose + 6 * k + c);
      r.push_back(p->aug);
      std::sort(r.begin(), r.end());
      dn[s_].m = (int)r.size();
      mmax = std::max(mmax, dn[s_].m);
      rows.insert(rows.end(), r.begin(), r.end());
      owner.insert(owner.end(), r.size(), s_);
    }
    p->sp_item0[l] = dn[lv.first[l]].row_off; p->sp_items[l] = (int)rows.size() - p->sp_item0[l];
    const int P = mmax * (mmax + 1) / 2;
    p->sp_tiles[l] = std::max(1, std::min(32, (P + 2047) / 2048));
    p->sp_shmem[l] = (9 * mmax + 81 + 9) * 8 + 2 * 4 * mmax + 16;
  }
  p->sp_levels = lv;
  hipStream_t q = p->ctx->stream;
  LVF_TRY(p->perm.assign(p->perm_h.data(), p->perm_h.size(), q)); LVF_TRY(p->iperm.assign(iperm.data(), iperm.size(), q));
  p->ldG = 0;
  if (ns) {
    rows_nat.resize(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) rows_nat[i] = iperm[rows[i]];
    LVF_TRY(p->sp_rows_nat.assign(rows_nat.data(), rows_nat.size(), q));
    LVF_TRY(p->sp_nodes.assign(dn.data(), dn.size(), q)); LVF_TRY(p->sp_rows.assign(rows.data(), rows.size(), q)); LVF_TRY(p->sp_owner.assign(owner.data(), owner.size(), q));
    LVF_TRY(p->sp_W.ensure(rows.size() * 9)); LVF_TRY(p->sp_L.ensure((size_t)ns * 81));
    p->sp_wstride = (int)rows.size();
    p->ldG = ((p->ndense + 1 + 15) / 16) * 16;
    std::vector<int> gmap((size_t)ns * p->ldG, -1);
    for (int s_ = 0; s_ < ns; ++s_)
      for (int r = 0; r < dn[s_].m; ++r) { const int R = rows[dn[s_].row_off + r]; if (R >= p->off) gmap[(size_t)s_ * p->ldG + (R - p->off)] = dn[s_].row_off + r; }
    LVF_TRY(p->sp_gmap.assign(gmap.data(), gmap.size(), q));
    LVF_HIP(hipStreamSynchronize(q));    // (gmap goes out of scope with this block)
  }
  LVF_HIP(hipStreamSynchronize(q));      // the host vectors above go out of scope
  p->plan_key = std::move(key);
  return LVF_OK;
}

int problem_configure(lvf_problem* p) {
  const bool cfg_timing = solver_env().configure_timing;
  const auto cfg_t0 = std::chrono::steady_clock::now();
  auto cfg_mark = [&](const char* what) {
    if (cfg_timing) std::fprintf(stderr, "  problem_configure: %s at %.3f ms\n", what, 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - cfg_t0).count());
  };
  lvf_state* st = p->st;
  lvf_ctx* ctx = p->ctx;
  p->n_kf = st->n_kf; p->n_lm = st->n_lm;
  p->d = 15 * p->n_kf; p->dp = 6 * p->n_kf;
  p->ldE = ((p->dp + 1 + 15) / 16) * 16;
  p->dpad = ((p->d + 1 + 63) / 64) * 64;
  LVF_TRY(build_elimination_plan(p));                 // sets ld, off, off_pose, ndense, aug, nb and the sparse levels
  cfg_mark("elimination plan");
  const size_t nS = (size_t)p->dpad * p->dpad;
  LVF_TRY(p->Dinv.ensure((size_t)p->nb * kNB * kNB)); LVF_TRY(p->Ldiag.ensure((size_t)p->nb * kNB * kNB));
  LVF_TRY(p->B.ensure(nS)); LVF_TRY(p->S.ensure((size_t)p->ld * p->ld)); LVF_TRY(p->gc.ensure(p->dpad)); LVF_TRY(p->dxc.ensure(p->dpad));
  LVF_TRY(p->C.ensure(p->n_lm)); LVF_TRY(p->gr.ensure(p->n_lm)); LVF_TRY(p->Cd.ensure(p->n_lm)); LVF_TRY(p->dxl.ensure(p->n_lm));
  LVF_TRY(p->scal.ensure(SC_ALLOC)); LVF_TRY(p->sp_sync.ensure(kSpMaxLevels));
  // candidate state x + dx (an accepted candidate is copied into the state by k_lm_decide)
  LVF_TRY(p->poses2.ensure(std::max(st->poses.cap, (size_t)7 * p->n_kf))); LVF_TRY(p->vel2.ensure(std::max(st->vel.cap, (size_t)3 * p->n_kf)));
  LVF_TRY(p->ba2.ensure(std::max(st->ba.cap, (size_t)3 * p->n_kf))); LVF_TRY(p->bg2.ensure(std::max(st->bg.cap, (size_t)3 * p->n_kf)));
  LVF_TRY(p->invd2.ensure(std::max(st->inv_depth.cap, (size_t)p->n_lm)));
  LVF_TRY(p->pose_const.ensure((size_t)p->n_kf + 8)); LVF_TRY(p->fail.ensure(1));      // (+8: cleared in 8-byte words)
  p->pose_const_h.assign(p->n_kf, 0);
  cfg_mark("buffers");
  p->tf_work.n = 0;
  p->tf_unique_lk2 = false; p->tf_k1_first = false; p->compact = false; p->tf_sorted_copy = false;
  lvf_batch* two_frame = p->tf;
  if (two_frame && two_frame->n && two_frame->sorted_by_kf && !two_frame->kf2_counts.empty() && two_frame->unique_lk2_known) {
    // the creator (the persistent window) vouches for the shape: sorted by current keyframe, k1 < k2, one block per (landmark, keyframe)
    size_t total = 0, nw = 0;
    for (int32_t c : two_frame->kf2_counts) { total += (size_t)c; nw += ((size_t)c + kT - 1) / kT; }
    if (total != (size_t)two_frame->n) { set_error("two-frame batch: per-keyframe counts do not add up to the number of blocks"); return LVF_ERR_INVALID; }
    LVF_TRY(p->h_tf_work.reserve(nw + 1));
    nw = 0;
    int at = 0;
    for (size_t k = 0; k < two_frame->kf2_counts.size(); ++k)
      for (int left = two_frame->kf2_counts[k]; left > 0; left -= kT) { const int c = std::min(left, kT); p->h_tf_work[nw++] = TfWork{at, c, (int)k}; at += c; }
    LVF_TRY(p->tf_work.assign(p->h_tf_work.p, nw, ctx->stream));
    p->tf_k1_first = true; p->tf_unique_lk2 = true;
  } else if (two_frame && two_frame->n && two_frame->sorted_by_kf && !two_frame->host_kf2.empty()) {
    // work list for the sorted fast path: runs of <= kT blocks sharing one current keyframe; k1 == k2 disables it.
    // ONE pass over the blocks gathers everything the host has to know about them (the list is 72 k entries at configs[3] and this
    // function is on adapt::Solve's path: seven separate passes were 0.45 ms of it):
    //   * k1 != k2 everywhere, k1 < k2 everywhere;
    //   * the current-keyframe runs (their starts) and, per run, how many blocks have which first keyframe (for the counting sort below);
    //   * how often the first keyframe steps DOWN inside a run (ids in creation order: almost never);
    //   * one block per (landmark, current keyframe) and ONE first keyframe per landmark, with two per-landmark tables: `seen_run[l]` =
    //     the last run landmark l appeared in (a repeat inside one run is a duplicate pair), `first_kf[l]` = its first keyframe.  The plain
    //     stores into E[l][k2 columns] must never meet the adds into E[l][k1 columns]; BuildProblem's blocks always satisfy this, a
    //     hand-made batch may not.
    const std::vector<int32_t>& k2 = two_frame->host_kf2; const std::vector<int32_t>& k1 = two_frame->host_kf1;
    const std::vector<int32_t>& lmh = two_frame->host_lm;
    const int n = two_frame->n, nkf = p->n_kf;
    const bool want_hist = solver_env().tf_k1sort && nkf <= 256;
    bool ok = true, k1_first = true;
    bool uniq = two_frame->unique_lk2_known || lmh.size() == (size_t)n;
    const bool check_uniq = uniq && !two_frame->unique_lk2_known;
    const int32_t nl = (int32_t)p->n_lm;
    std::vector<int32_t> seen_run, first_kf;
    if (check_uniq) { seen_run.assign((size_t)nl, -1); first_kf.assign((size_t)nl, -1); }
    std::vector<int32_t> run_start;                 // first block of every current-keyframe run (+ n at the end)
    std::vector<int32_t> hist;                      // [run][first keyframe] block counts
    run_start.reserve((size_t)nkf + 2);
    if (want_hist) hist.reserve((size_t)(nkf + 1) * nkf);
    int descents = 0, cur = INT32_MIN, run = -1;
    int32_t* hrow = nullptr;
    for (int i = 0; i < n; ++i) {
      const int a = k1[i], c2 = k2[i];
      ok = ok && a != c2; k1_first = k1_first && a < c2;
      if (c2 != cur) {
        cur = c2; ++run; run_start.push_back(i);
        if (want_hist) { hist.resize(hist.size() + (size_t)nkf, 0); hrow = hist.data() + (size_t)run * nkf; }
      } else descents += a < k1[i - 1] ? 1 : 0;
      if (want_hist) ++hrow[std::min(std::max(a, 0), nkf - 1)];
      if (check_uniq && uniq) {
        const int32_t l = lmh[i];
        if (l < 0 || l >= nl) uniq = false;
        else {
          if (seen_run[l] == run) uniq = false;
          seen_run[l] = run;
          if (first_kf[l] < 0) first_kf[l] = a; else if (first_kf[l] != a) uniq = false;
        }
      }
    }
    run_start.push_back(n);
    p->tf_k1_first = ok && k1_first;
    if (ok) {
      // built straight into pinned staging owned by the problem: the upload is a real asynchronous copy and this function does not
      // have to wait for the stream before returning
      size_t nw = 0;
      for (size_t r = 0; r + 1 < run_start.size(); ++r) nw += (size_t)(run_start[r + 1] - run_start[r] + kT - 1) / kT;
      LVF_TRY(p->h_tf_work.reserve(nw + 1));
      nw = 0;
      for (size_t r = 0; r + 1 < run_start.size(); ++r)
        for (int i = run_start[r]; i < run_start[r + 1]; i += kT) p->h_tf_work[nw++] = TfWork{i, std::min(kT, run_start[r + 1] - i), k2[run_start[r]]};
      LVF_TRY(p->tf_work.assign(p->h_tf_work.p, nw, ctx->stream));
      // first keyframes out of order inside the runs (more than one block in eight steps DOWN): sorted copies for the linearisation.
      // BuildProblem's own order (landmark ids in creation order) passes untouched.
      if (want_hist && (size_t)descents * 8 > (size_t)n) {
        LVF_TRY(p->h_tfs_perm.reserve((size_t)n));
        int* perm = p->h_tfs_perm.p;
        for (size_t r = 0; r + 1 < run_start.size(); ++r) {     // counting sort of each run by first keyframe (stable): the histogram is there
          int32_t* cnt = hist.data() + r * (size_t)nkf;
          int32_t at = run_start[r];
          for (int k = 0; k < nkf; ++k) { const int32_t c = cnt[k]; cnt[k] = at; at += c; }
          for (int t = run_start[r]; t < run_start[r + 1]; ++t) perm[cnt[std::min(std::max(k1[t], 0), nkf - 1)]++] = t;
        }
        LVF_TRY(p->tfs_perm.assign(perm, (size_t)n, ctx->stream));
        LVF_TRY(p->tfs_fo.ensure(n)); LVF_TRY(p->tfs_ob.ensure(n)); LVF_TRY(p->tfs_lm.ensure(n)); LVF_TRY(p->tfs_k1.ensure(n)); LVF_TRY(p->tfs_k2.ensure(n));
        hipLaunchKernelGGL(k_tf_gather, dim3(grid(n)), dim3(kT), 0, ctx->stream, n, p->tfs_perm.p, (const double2*)two_frame->ob_a.p, (const double2*)two_frame->ob_b.p,
                           two_frame->idx_a.p, two_frame->idx_b.p, two_frame->idx_c.p, p->tfs_fo.p, p->tfs_ob.p, p->tfs_lm.p, p->tfs_k1.p, p->tfs_k2.p);
        LVF_HIP(hipGetLastError());
        p->tf_sorted_copy = true;
      }
      p->tf_unique_lk2 = uniq;
    }
  }
  cfg_mark("TwoFrame work list + shape checks");
  // landmark tracks -> band-limited Schur (device side: the TwoFrame indices already live there)
  p->band_ready = false;
  const bool band_ok = solver_env().schur_band && p->n_lm > 0 && (size_t)(4 * p->n_kf + 1) * sizeof(int) <= 48 * 1024;
  // compact landmark layout + slabs (atomic-free TwoFrame linearisation): needs the sorted work list, one block per (landmark,
  // keyframe), the landmark's first keyframe ahead of its observations, and the merged band-Schur launch
  const size_t shb = ((size_t)kSchurRows * (p->ldE + 16) + kSchurRows) * sizeof(double) + kBandRowsMax * sizeof(int);
  const bool merged = shb <= 64 * 1024 && p->sp_levels.n > 0 && (size_t)p->sp_shmem[0] <= 64 * 1024;
  const bool want_compact = band_ok && solver_env().compact && merged && p->dp <= 320 && two_frame && two_frame->n && p->tf_work.n && p->n_kf <= kMaxStagedKf && p->tf_unique_lk2 && p->tf_k1_first;
  LVF_TRY(p->E.ensure((size_t)p->n_lm * p->ldE));
  if (band_ok) { LVF_TRY(p->lm_kmin.ensure(p->n_lm)); LVF_TRY(p->lm_kmax.ensure(p->n_lm)); LVF_TRY(p->lm_order.ensure(p->n_lm)); LVF_TRY(p->lm_nactive.ensure(1)); }
  // atomic-free mode: E's non-zero pattern is fixed for the problem and fully overwritten by every linearisation — cleared once, here;
  // one launch for the clears AND the landmark tracks' initial values (a persistent window reconfigures every tick)
  {
    ZeroList z{};
    if (want_compact && p->n_lm) { z.p[z.count] = p->E.p; z.n[z.count] = (unsigned long long)p->n_lm * p->ldE; ++z.count; }
    z.p[z.count] = reinterpret_cast<double*>(p->pose_const.p); z.n[z.count] = (unsigned long long)(p->n_kf + 7) / 8; ++z.count;      // (the buffer's capacity is padded)
    z.p[z.count] = p->dxc.p; z.n[z.count] = (unsigned long long)p->dpad; ++z.count;
    hipLaunchKernelGGL(k_zero_multi_ranges, dim3(512, z.count + (band_ok ? 1 : 0)), dim3(kT), 0, ctx->stream, z, p->n_lm, band_ok ? p->lm_kmin.p : nullptr, band_ok ? p->lm_kmax.p : nullptr);
    LVF_HIP(hipGetLastError());
  }
  if (band_ok) {
    hipStream_t q = ctx->stream;
    if (two_frame && two_frame->n)
      hipLaunchKernelGGL(k_lm_range, dim3(grid(two_frame->n)), dim3(kT), 0, q, two_frame->n, two_frame->idx_a.p, two_frame->idx_b.p, two_frame->idx_c.p,
                         p->lm_kmin.p, p->lm_kmax.p);
    if (want_compact) {
      LVF_TRY(p->lm_eoff.ensure(p->n_lm)); LVF_TRY(p->n_slots.ensure(1));
      // (the slot offsets ride beside the sort: two independent one-workgroup chains, one launch)
      hipLaunchKernelGGL(k_lm_sort_offsets, dim3(2), dim3(1024), (size_t)(4 * p->n_kf + 1) * sizeof(int), q, p->n_lm, p->n_kf, p->lm_kmin.p, p->lm_kmax.p, p->lm_order.p,
                         p->lm_nactive.p, p->lm_eoff.p, p->n_slots.p);
    } else
    hipLaunchKernelGGL(k_lm_sort, dim3(1), dim3(1024), (size_t)(4 * p->n_kf + 1) * sizeof(int), q, p->n_lm, p->n_kf, p->lm_kmin.p, p->lm_kmax.p, p->lm_order.p,
                       p->lm_nactive.p);
    LVF_HIP(hipGetLastError());
    p->band_ready = true;
    p->band_rows_built = 0;         // the bands changed: the work list is rebuilt with the next chain
    p->band_epoch += 1;
    if (want_compact) {
      const size_t cap_slots = (size_t)p->n_lm * (size_t)std::max(p->n_kf - 1, 1);      // worst case: every landmark seen by every later keyframe
      const int n_wg = (int)p->tf_work.n;
      LVF_TRY(p->tf_slot.ensure(two_frame->n));
      LVF_TRY(p->slotB.ensure(cap_slots * 8));
      LVF_TRY(p->Ct.ensure(p->n_lm)); LVF_TRY(p->grt.ensure(p->n_lm));
      LVF_TRY(p->slabP.ensure((size_t)n_wg * p->n_kf * kSlabRow)); LVF_TRY(p->slabQ.ensure((size_t)n_wg * kSlabQ));
      {
        const int g_slots = grid(two_frame->n);
        hipLaunchKernelGGL(k_tf_slots_zero, dim3(g_slots + 256), dim3(kT), 0, q, two_frame->n, g_slots, p->tf_lm(), p->tf_k2(), p->lm_kmin.p, p->lm_eoff.p, p->tf_slot.p,
                           p->n_slots.p, p->slotB.p);
      }
      LVF_HIP(hipGetLastError());
      // run_first[k] = first workgroup of current keyframe k's run (the work list is sorted by k2); run_first[n_kf] = n_wg
      LVF_TRY(p->h_run_first.reserve((size_t)p->n_kf + 1));
      {
        int w = 0;
        for (int k = 0; k <= p->n_kf; ++k) {
          while (w < n_wg && p->h_tf_work[w].k2 < k) ++w;
          p->h_run_first[k] = w;
        }
      }
      LVF_TRY(p->run_first.assign(p->h_run_first.p, (size_t)p->n_kf + 1, q));
      p->compact = true;
    }
  }
  cfg_mark("device-side layout launches + E");
  // no stream wait here: every host source above is pinned and owned by the problem (or was waited for by the plan builder)
  p->linearized = false;
  p->chain_ready = false;
  p->step_ready = false;
  return LVF_OK;
}

int problem_configure(lvf_problem* p, lvf_dense_prior* prior) {
  p->dprior = prior;
  return problem_configure(p);
}

// lvf_problem_set_dense_prior: the prior's keyframes are part of the elimination plan's key, so a change of that set configures the problem
// again (the constant flags, which a configure clears, are put back); the same set only swaps the pointer
int problem_set_dense_prior(lvf_problem* p, lvf_dense_prior* prior) {
  // (the prior attached so far is borrowed and may be gone already: what it sat on is read from the plan's key, never from the object)
  std::vector<int32_t> was, now;
  const auto mark = std::find(p->plan_key.begin(), p->plan_key.end(), INT32_MIN);
  if (mark != p->plan_key.end()) was.assign(mark + 1, p->plan_key.end());
  if (prior) now = prior->kf_h;
  std::sort(now.begin(), now.end());
  p->dprior = prior;
  p->linearized = false;
  p->chain_ready = false;
  if (was == now && p->n_kf == p->st->n_kf) return LVF_OK;
  const std::vector<uint8_t> bits = p->pose_const_h;
  LVF_TRY(problem_configure(p));
  if (bits.size() == p->pose_const_h.size() && !bits.empty()) {
    p->pose_const_h = bits;
    LVF_HIP(hipMemcpyAsync(p->pose_const.p, p->pose_const_h.data(), p->pose_const_h.size(), hipMemcpyHostToDevice, p->ctx->stream));
    LVF_HIP(hipStreamSynchronize(p->ctx->stream));
  }
  return LVF_OK;
}

}  // namespace lvf
