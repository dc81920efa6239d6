// reloc_hostcheck.cpp — stand-alone host-side check of csrc/reloc_kernels.hip: the option defaults and every argument check of
// lvf_orb_match / lvf_pnp_ransac / lvf_relocate_by_image / lvf_pnp_debug_hypotheses, plus the early returns that write the caller's arrays
// on the host.  Needs no GPU: the library's services (lvf::enter, set_error, ...) are stubbed below and enter() refuses, so nothing is ever
// launched.  Meant to be built with the host sanitizers and run on a CPU box:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fno-fast-math -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude lvio_fusion_amd/csrc/reloc_kernels.hip lvio_fusion_amd/host/reloc_hostcheck.cpp -o lvio_fusion_amd/host/reloc_hostcheck
//   lvio_fusion_amd/host/reloc_hostcheck          # prints "reloc_hostcheck: N checks passed", exit status 0
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../csrc/lvf_internal.hpp"

namespace lvf {
static std::string g_last;
thread_local std::shared_ptr<Pool> g_pool;
void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last = buf;
}
int hip_fail(hipError_t, const char*, const char*, int) { return LVF_ERR_HIP; }
int enter(lvf_ctx*) { set_error("host check: no device"); return LVF_ERR_NO_DEVICE; }
int device_scan1(lvf_ctx*, const int*, int, const int*, int*, int*, const float4*, float4*) { return LVF_ERR_NO_DEVICE; }
void make_camd(const lvf_camera&, CamD&) {}
}  // namespace lvf

static int g_checks = 0, g_failed = 0;
#define EXPECT(cond)                                                                             \
  do {                                                                                           \
    ++g_checks;                                                                                  \
    if (!(cond)) { ++g_failed; std::fprintf(stderr, "FAILED line %d: %s  (last error: %s)\n", __LINE__, #cond, lvf::g_last.c_str()); } \
  } while (0)

int main() {
  lvf_ctx* ctx = reinterpret_cast<lvf_ctx*>(new char[sizeof(void*)]);      // never dereferenced: enter() is stubbed
  const double nan = std::numeric_limits<double>::quiet_NaN();
  // defaults
  lvf_match_options mo;
  std::memset(&mo, 0xff, sizeof(mo));
  lvf_match_options_default(&mo);
  EXPECT(mo.max_distance == 50 && mo.ratio == 0.8f && mo.cross_check == 1);
  lvf_match_options_default(nullptr);
  lvf_pnp_options po;
  std::memset(&po, 0xff, sizeof(po));
  lvf_pnp_options_default(&po);
  EXPECT(po.num_hypotheses == 512 && po.seed == 0u && po.max_reproj_px == 3.0 && po.min_matches == 21 && po.refine_rounds == 2 && po.refine_iterations == 10 &&
         po.huber_a == 1.0);
  lvf_pnp_options_default(nullptr);

  // lvf_orb_match
  const int nq = 5, nt = 4;
  std::vector<uint8_t> qd(32 * nq, 1), td(32 * nt, 2);
  std::vector<int32_t> m(nq, 7), b(nq, 7), s(nq, 7);
  EXPECT(lvf_orb_match(nullptr, nq, qd.data(), nt, td.data(), nullptr, m.data(), nullptr, nullptr) == LVF_ERR_INVALID);
  EXPECT(lvf_orb_match(ctx, -1, qd.data(), nt, td.data(), nullptr, m.data(), nullptr, nullptr) == LVF_ERR_INVALID);
  EXPECT(lvf_orb_match(ctx, 8193, qd.data(), nt, td.data(), nullptr, m.data(), nullptr, nullptr) == LVF_ERR_INVALID);
  EXPECT(lvf_orb_match(ctx, nq, qd.data(), 8193, td.data(), nullptr, m.data(), nullptr, nullptr) == LVF_ERR_INVALID);
  EXPECT(lvf_orb_match(ctx, nq, nullptr, nt, td.data(), nullptr, m.data(), nullptr, nullptr) == LVF_ERR_INVALID);
  EXPECT(lvf_orb_match(ctx, nq, qd.data(), nt, nullptr, nullptr, m.data(), nullptr, nullptr) == LVF_ERR_INVALID);
  EXPECT(lvf_orb_match(ctx, nq, qd.data(), nt, td.data(), nullptr, nullptr, nullptr, nullptr) == LVF_ERR_INVALID);
  lvf_match_options bad = mo;
  bad.max_distance = -1;
  EXPECT(lvf_orb_match(ctx, nq, qd.data(), nt, td.data(), &bad, m.data(), nullptr, nullptr) == LVF_ERR_INVALID);
  bad = mo; bad.ratio = std::numeric_limits<float>::quiet_NaN();
  EXPECT(lvf_orb_match(ctx, nq, qd.data(), nt, td.data(), &bad, m.data(), nullptr, nullptr) == LVF_ERR_INVALID);
  bad = mo; bad.cross_check = 2;
  EXPECT(lvf_orb_match(ctx, nq, qd.data(), nt, td.data(), &bad, m.data(), nullptr, nullptr) == LVF_ERR_INVALID);
  EXPECT(lvf_orb_match(ctx, 0, nullptr, nt, td.data(), nullptr, nullptr, nullptr, nullptr) == LVF_OK);                // nq == 0: at once
  EXPECT(lvf_orb_match(ctx, nq, qd.data(), 0, nullptr, nullptr, m.data(), b.data(), s.data()) == LVF_OK);             // nt == 0: no match, on the host
  bool all_minus = true;
  for (int i = 0; i < nq; ++i) all_minus = all_minus && m[i] == -1 && b[i] == -1 && s[i] == -1;
  EXPECT(all_minus);
  EXPECT(lvf_orb_match(ctx, nq, qd.data(), 0, nullptr, nullptr, m.data(), nullptr, nullptr) == LVF_OK);               // best / second may be NULL
  EXPECT(lvf_orb_match(ctx, nq, qd.data(), nt, td.data(), nullptr, m.data(), b.data(), s.data()) == LVF_ERR_NO_DEVICE);      // every check passed

  // lvf_pnp_ransac
  lvf_camera cam{};
  cam.fx = 458.0; cam.fy = 457.0; cam.cx = 367.0; cam.cy = 248.0; cam.extrinsic[3] = 1.0;
  const int n = 30;
  std::vector<double> pw(3 * n, 1.0);
  std::vector<float> pt(2 * n, 10.f);
  std::vector<uint8_t> inl(n, 9);
  double pose[7] = {0, 0, 0, 1, 0, 0, 0}, init[7] = {0, 0, 0, 1, 0, 0, 0};
  int32_t score = -5;
  lvf_solver_summary summ;
  EXPECT(lvf_pnp_ransac(nullptr, &cam, n, pw.data(), pt.data(), nullptr, nullptr, pose, &score, inl.data(), &summ) == LVF_ERR_INVALID);
  EXPECT(lvf_pnp_ransac(ctx, &cam, n, pw.data(), pt.data(), nullptr, nullptr, pose, nullptr, inl.data(), &summ) == LVF_ERR_INVALID);
  EXPECT(lvf_pnp_ransac(ctx, &cam, -1, pw.data(), pt.data(), nullptr, nullptr, pose, &score, inl.data(), &summ) == LVF_ERR_INVALID);
  EXPECT(lvf_pnp_ransac(ctx, &cam, 8193, pw.data(), pt.data(), nullptr, nullptr, pose, &score, nullptr, &summ) == LVF_ERR_INVALID);
  EXPECT(lvf_pnp_ransac(ctx, nullptr, n, pw.data(), pt.data(), nullptr, nullptr, pose, &score, inl.data(), &summ) == LVF_ERR_INVALID);
  EXPECT(lvf_pnp_ransac(ctx, &cam, n, nullptr, pt.data(), nullptr, nullptr, pose, &score, inl.data(), &summ) == LVF_ERR_INVALID);
  EXPECT(lvf_pnp_ransac(ctx, &cam, n, pw.data(), nullptr, nullptr, nullptr, pose, &score, inl.data(), &summ) == LVF_ERR_INVALID);
  EXPECT(lvf_pnp_ransac(ctx, &cam, n, pw.data(), pt.data(), nullptr, nullptr, nullptr, &score, inl.data(), &summ) == LVF_ERR_INVALID);
  lvf_camera badcam = cam;
  badcam.fx = 0.0;
  EXPECT(lvf_pnp_ransac(ctx, &badcam, n, pw.data(), pt.data(), nullptr, nullptr, pose, &score, inl.data(), &summ) == LVF_ERR_INVALID);
  badcam = cam; badcam.extrinsic[3] = 0.0;                                                                             // zero quaternion
  EXPECT(lvf_pnp_ransac(ctx, &badcam, n, pw.data(), pt.data(), nullptr, nullptr, pose, &score, inl.data(), &summ) == LVF_ERR_INVALID);
  double badinit[7] = {0, 0, 0, 1, nan, 0, 0};
  EXPECT(lvf_pnp_ransac(ctx, &cam, n, pw.data(), pt.data(), badinit, nullptr, pose, &score, inl.data(), &summ) == LVF_ERR_INVALID);
  lvf_pnp_options pb = po;
  pb.num_hypotheses = 0;
  EXPECT(lvf_pnp_ransac(ctx, &cam, n, pw.data(), pt.data(), nullptr, &pb, pose, &score, inl.data(), &summ) == LVF_ERR_INVALID);
  pb = po; pb.num_hypotheses = 4097;
  EXPECT(lvf_pnp_ransac(ctx, &cam, n, pw.data(), pt.data(), nullptr, &pb, pose, &score, inl.data(), &summ) == LVF_ERR_INVALID);
  pb = po; pb.max_reproj_px = 0.0;
  EXPECT(lvf_pnp_ransac(ctx, &cam, n, pw.data(), pt.data(), nullptr, &pb, pose, &score, inl.data(), &summ) == LVF_ERR_INVALID);
  pb = po; pb.min_matches = 2;
  EXPECT(lvf_pnp_ransac(ctx, &cam, n, pw.data(), pt.data(), nullptr, &pb, pose, &score, inl.data(), &summ) == LVF_ERR_INVALID);
  pb = po; pb.refine_rounds = -1;
  EXPECT(lvf_pnp_ransac(ctx, &cam, n, pw.data(), pt.data(), nullptr, &pb, pose, &score, inl.data(), &summ) == LVF_ERR_INVALID);
  pb = po; pb.huber_a = nan;
  EXPECT(lvf_pnp_ransac(ctx, &cam, n, pw.data(), pt.data(), nullptr, &pb, pose, &score, inl.data(), &summ) == LVF_ERR_INVALID);
  // the early exit: 20 < min_matches, nothing launched, score 0, mask cleared, pose untouched
  pose[4] = 42.0; score = -5;
  EXPECT(lvf_pnp_ransac(ctx, &cam, 20, pw.data(), pt.data(), init, nullptr, pose, &score, inl.data(), &summ) == LVF_OK);
  bool cleared = true;
  for (int i = 0; i < 20; ++i) cleared = cleared && inl[i] == 0;
  EXPECT(score == 0 && cleared && inl[20] == 9 && pose[4] == 42.0 && summ.num_iterations == 0);
  EXPECT(lvf_pnp_ransac(ctx, &cam, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &score, nullptr, nullptr) == LVF_OK);
  EXPECT(lvf_pnp_ransac(ctx, &cam, n, pw.data(), pt.data(), init, nullptr, pose, &score, inl.data(), &summ) == LVF_ERR_NO_DEVICE);

  // lvf_relocate_by_image
  const int n_old = 25, n_cur = 28;
  std::vector<double> opw(3 * n_old, 2.0);
  std::vector<uint8_t> od(32 * n_old, 3), cd(32 * n_cur, 4), cin(n_cur, 9);
  std::vector<float> cpt(2 * n_cur, 5.f);
  std::vector<int32_t> cm(n_cur, 7);
  double old_pose[7] = {0, 0, 0, 1, 1, 2, 3}, rel[7] = {0, 0, 0, 2, 0.5, 0, 0};
  EXPECT(lvf_relocate_by_image(nullptr, &cam, old_pose, n_old, opw.data(), od.data(), n_cur, cpt.data(), cd.data(), nullptr, nullptr, rel, &score, cm.data(), cin.data(),
                               &summ) == LVF_ERR_INVALID);
  EXPECT(lvf_relocate_by_image(ctx, &cam, nullptr, n_old, opw.data(), od.data(), n_cur, cpt.data(), cd.data(), nullptr, nullptr, rel, &score, cm.data(), cin.data(), &summ) ==
         LVF_ERR_INVALID);
  EXPECT(lvf_relocate_by_image(ctx, &cam, old_pose, n_old, opw.data(), od.data(), n_cur, cpt.data(), cd.data(), nullptr, nullptr, nullptr, &score, cm.data(), cin.data(),
                               &summ) == LVF_ERR_INVALID);
  EXPECT(lvf_relocate_by_image(ctx, &cam, old_pose, n_old, opw.data(), od.data(), n_cur, cpt.data(), cd.data(), nullptr, nullptr, rel, nullptr, cm.data(), cin.data(), &summ) ==
         LVF_ERR_INVALID);
  EXPECT(lvf_relocate_by_image(ctx, &cam, old_pose, 8193, opw.data(), od.data(), n_cur, cpt.data(), cd.data(), nullptr, nullptr, rel, &score, nullptr, nullptr, &summ) ==
         LVF_ERR_INVALID);
  EXPECT(lvf_relocate_by_image(ctx, &cam, old_pose, n_old, nullptr, od.data(), n_cur, cpt.data(), cd.data(), nullptr, nullptr, rel, &score, cm.data(), cin.data(), &summ) ==
         LVF_ERR_INVALID);
  EXPECT(lvf_relocate_by_image(ctx, &cam, old_pose, n_old, opw.data(), od.data(), n_cur, nullptr, cd.data(), nullptr, nullptr, rel, &score, cm.data(), cin.data(), &summ) ==
         LVF_ERR_INVALID);
  double zero_q[7] = {0, 0, 0, 0, 0, 0, 0};
  EXPECT(lvf_relocate_by_image(ctx, &cam, zero_q, n_old, opw.data(), od.data(), n_cur, cpt.data(), cd.data(), nullptr, nullptr, rel, &score, cm.data(), cin.data(), &summ) ==
         LVF_ERR_INVALID);
  EXPECT(lvf_relocate_by_image(ctx, &cam, old_pose, n_old, opw.data(), od.data(), n_cur, cpt.data(), cd.data(), &bad, nullptr, rel, &score, cm.data(), cin.data(), &summ) ==
         LVF_ERR_INVALID);
  EXPECT(lvf_relocate_by_image(ctx, &cam, old_pose, n_old, opw.data(), od.data(), n_cur, cpt.data(), cd.data(), nullptr, &pb, rel, &score, cm.data(), cin.data(), &summ) ==
         LVF_ERR_INVALID);
  // an empty old frame: nothing to match, rejected on the host, relative_o_c untouched
  score = -5;
  EXPECT(lvf_relocate_by_image(ctx, &cam, old_pose, 0, nullptr, nullptr, n_cur, cpt.data(), cd.data(), nullptr, nullptr, rel, &score, cm.data(), cin.data(), &summ) ==
         LVF_OK);
  bool none = true;
  for (int i = 0; i < n_cur; ++i) none = none && cm[i] == -1 && cin[i] == 0;
  EXPECT(score == 0 && none && rel[3] == 2.0 && rel[4] == 0.5);
  EXPECT(lvf_relocate_by_image(ctx, &cam, old_pose, n_old, opw.data(), od.data(), 0, nullptr, nullptr, nullptr, nullptr, rel, &score, nullptr, nullptr, nullptr) == LVF_OK);
  EXPECT(lvf_relocate_by_image(ctx, &cam, old_pose, n_old, opw.data(), od.data(), n_cur, cpt.data(), cd.data(), nullptr, nullptr, rel, &score, cm.data(), cin.data(), &summ) ==
         LVF_ERR_NO_DEVICE);

  // lvf_pnp_debug_hypotheses
  std::vector<int32_t> tri(3 * 512), npo(512), cnt(512);
  EXPECT(lvf_pnp_debug_hypotheses(ctx, &cam, 2, pw.data(), pt.data(), nullptr, tri.data(), npo.data(), cnt.data(), nullptr) == LVF_ERR_INVALID);
  EXPECT(lvf_pnp_debug_hypotheses(ctx, &cam, n, pw.data(), pt.data(), nullptr, nullptr, npo.data(), cnt.data(), nullptr) == LVF_ERR_INVALID);
  EXPECT(lvf_pnp_debug_hypotheses(ctx, &cam, n, pw.data(), pt.data(), &pb, tri.data(), npo.data(), cnt.data(), nullptr) == LVF_ERR_INVALID);
  EXPECT(lvf_pnp_debug_hypotheses(ctx, &cam, n, pw.data(), pt.data(), nullptr, tri.data(), npo.data(), cnt.data(), nullptr) == LVF_ERR_NO_DEVICE);

  delete[] reinterpret_cast<char*>(ctx);
  if (g_failed) { std::fprintf(stderr, "reloc_hostcheck: %d of %d checks FAILED\n", g_failed, g_checks); return 1; }
  std::printf("reloc_hostcheck: %d checks passed\n", g_checks);
  return 0;
}
