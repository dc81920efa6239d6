"""GPU parity of the image undistortion (lvio_fusion_amd/csrc/undistort_kernels.hip) through the C-ABI against the CPU restatement
tests/undistort_ref.py (itself checked against an exact rational model, fp64 bilinear interpolation and analytic truth in
tests/test_undistort_ref.py).  Everything is integer from the map on, so every comparison is bit equality:
  * the downloaded map against the restatement's;
  * level 0 of the undistorted image against the restatement's remap, at sizes that take the scalar tail ((w * h) % 4 != 0), less than one
    wave, several workgroups, a padded row stride, and with sets that send waves down both the checked and the unchecked path;
  * everything after level 0 against lvf_image_create of the restatement's output (the existing call is the yardstick there);
  * the pair call against two single calls, and against itself.
No test provokes a device fault: every refusal is decided on the host before a launch."""
import numpy as np
import pytest

from tests import klt_cases as kc
from tests import undistort_cases as uc
from tests import undistort_ref as ur

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


def same_image(a, b, what):
    assert a.size() == b.size(), what
    for L in range(a.levels):
        (ga, da), (gb, db) = a.level(L), b.level(L)
        assert np.array_equal(ga, gb), f"{what}: gray level {L}"
        assert np.array_equal(da, db), f"{what}: derivative level {L}"


@pytest.mark.parametrize("w,h", [(67, 45), (253, 131)])
@pytest.mark.parametrize("name", list(uc.SETS))
def test_map_download_bit_equal(ctx, w, h, name):
    from lvio_fusion_amd import api
    cam = uc.camera(w, h)
    u = api.Undistort(ctx, cam, uc.SETS[name], w, h)
    xy, frac = u.map()
    rxy, rfrac = ur.build_map(cam, uc.SETS[name], w, h)
    assert np.array_equal(xy, rxy) and np.array_equal(frac, rfrac)
    u.close()


@pytest.mark.parametrize("w,h,pad,names", [(1, 1, 0, ("barrel", "pincushion")), (5, 3, 0, ("barrel", "pincushion")), (67, 45, 0, ("barrel", "pincushion")),
                                           (253, 131, 0, ("barrel", "pincushion")), (640, 376, 24, ("barrel", "pincushion")), (1241, 376, 0, ("barrel",))])
def test_level0_bit_equal(ctx, w, h, pad, names):
    from lvio_fusion_amd import api
    cam = uc.camera(w, h)
    raw = uc.raw_image(w, h, pad=pad)
    for name in names:
        xy, frac = ur.build_map(cam, uc.SETS[name], w, h)
        want = ur.remap(np.ascontiguousarray(raw), xy, frac)
        border, full = ur.coverage(xy, w, h)
        u = api.Undistort(ctx, cam, uc.SETS[name], w, h)
        img = u.image(raw, 0)
        got = img.level(0)[0]
        print(f"{w} x {h} {name}: {100 * border:.1f} % of the pixels have a tap outside, {int((got != want).sum())} differ")
        assert got.shape == want.shape and np.array_equal(got, want), f"{w} x {h} {name}"
        if w >= 67:
            assert border >= 0.01 and full >= 0.5                      # both paths of the kernel ran
        img.close(); u.close()


def test_whole_image_equals_image_create_of_the_restatement(ctx):
    from lvio_fusion_amd import api
    w, h = 253, 131
    cam, raw = uc.camera(w, h), uc.raw_image(w, h, seed=2)
    u = api.Undistort(ctx, cam, uc.EUROC, w, h)
    a, b = u.image(raw, 3), api.Image(ctx, ur.undistort(raw, cam, uc.EUROC), 3)
    assert a.size() == (w, h, 4)
    same_image(a, b, "undistorted image")
    a.close(); b.close(); u.close()


def test_pair_equals_two_single_calls_and_itself(ctx):
    from lvio_fusion_amd import api
    w, h = 253, 131
    cam0, cam1 = uc.camera(w, h), uc.camera(w, h, f=0.27)
    raw0, raw1 = uc.raw_image(w, h, seed=4), uc.raw_image(w, h, seed=5, pad=9)
    u0, u1 = api.Undistort(ctx, cam0, uc.EUROC, w, h), api.Undistort(ctx, cam1, uc.PINCUSHION, w, h)
    p0, p1 = u0.pair(u1, raw0, raw1, 3)
    q0, q1 = u0.pair(u1, raw0, raw1, 3)
    s0, s1 = u0.image(raw0, 3), u1.image(raw1, 3)
    same_image(p0, s0, "pair, camera 0"); same_image(p1, s1, "pair, camera 1")
    same_image(p0, q0, "pair run twice, camera 0"); same_image(p1, q1, "pair run twice, camera 1")
    assert not np.array_equal(p0.level(0)[0], p1.level(0)[0])
    # one map for both frames (one camera model): the frames share its staging buffer and must not mix
    r0, r1 = u0.pair(u0, raw0, raw1, 3)
    t1 = u0.image(raw1, 3)
    same_image(r0, s0, "shared map, frame 0"); same_image(r1, t1, "shared map, frame 1")
    for x in (p0, p1, q0, q1, s0, s1, r0, r1, t1, u0, u1):
        x.close()


@pytest.mark.parametrize("w,h", [(67, 45), (1241, 376)])
def test_zero_distortion_equals_image_create(ctx, w, h):
    from lvio_fusion_amd import api
    cam, raw = uc.camera(w, h), uc.raw_image(w, h, seed=6)
    plain = api.Image(ctx, raw, 3)
    for dist in (None, uc.ZERO):
        u = api.Undistort(ctx, cam, dist, w, h)
        img = u.image(raw, 3)
        same_image(img, plain, f"zero distortion ({dist})")
        img.close(); u.close()
    plain.close()


def test_downstream_consumers_take_the_images_unchanged(ctx):
    """an undistorted pair through lvf_stereo_triangulate and lvf_orb_detect: the same arrays as with lvf_image_create(restatement(raw))"""
    from lvio_fusion_amd import api
    c = kc.stereo_case(21, n=300)
    w, h = kc.W, kc.H
    yy, xx = np.mgrid[0:h, 0:w]
    checker = (40 * ((xx // 17 + yy // 13) % 2)).astype(np.int32)          # corners for FAST
    raw0 = np.clip(c["left"].astype(np.int32) + checker - 20, 0, 255).astype(np.uint8)
    raw1 = c["right"]
    dist = (-0.05, 0.01, 5e-4, -3e-4)                                      # mild: the scene survives, so the consumers have work to do
    u0, u1 = api.Undistort(ctx, c["cam0"], dist, w, h), api.Undistort(ctx, c["cam1"], dist, w, h)
    left, right = u0.pair(u1, c["left"], raw1, 3)
    ref_l, ref_r = api.Image(ctx, ur.undistort(c["left"], c["cam0"], dist), 3), api.Image(ctx, ur.undistort(raw1, c["cam1"], dist), 3)
    got = api.stereo_triangulate(left, right, c["cam0"], c["cam1"], c["baseline"], c["kps"])
    want = api.stereo_triangulate(ref_l, ref_r, c["cam0"], c["cam1"], c["baseline"], c["kps"])
    assert all(np.array_equal(g.view(np.uint8), r.view(np.uint8)) for g, r in zip(got, want))
    assert (got[1] == 1).sum() > 100
    orb = api.Orb(ctx, api.orb_options(num_features=200))
    img, ref = u0.image(raw0, 0), api.Image(ctx, ur.undistort(raw0, c["cam0"], dist), 0)
    k_got, k_want = orb.detect(img), orb.detect(ref)
    assert all(np.array_equal(k_got[k].view(np.uint8), k_want[k].view(np.uint8)) for k in k_want)
    assert len(k_got["pt"]) >= 20
    for x in (left, right, ref_l, ref_r, img, ref, orb, u0, u1):
        x.close()


def test_refusals(ctx):
    from lvio_fusion_amd import api
    w, h = 67, 45
    cam, raw = uc.camera(w, h), uc.raw_image(w, h)
    for bad_cam, dist, bw, bh in [(dict(cam, fx=0.0), uc.BARREL, w, h), (dict(cam, fy=-1.0), uc.BARREL, w, h), (cam, (0.1, float("nan"), 0.0, 0.0), w, h),
                                  (cam, (float("inf"), 0.0, 0.0, 0.0), w, h), (cam, uc.BARREL, 4097, 8), (cam, uc.BARREL, 8, 4097), (cam, uc.BARREL, 0, 8)]:
        with pytest.raises(api.LvfError) as e:
            api.Undistort(ctx, bad_cam, dist, bw, bh)
        assert "lvf error 1:" in str(e.value) and "lvf_undistort_create" in str(e.value)
    u = api.Undistort(ctx, cam, uc.BARREL, w, h)
    other = api.Undistort(ctx, uc.camera(w + 1, h), uc.BARREL, w + 1, h)
    for call in (lambda: u.image(uc.raw_image(w + 1, h), 0), lambda: u.image(uc.raw_image(w, h - 1), 0), lambda: u.image(raw, 8),
                 lambda: u.pair(other, raw, raw, 0), lambda: other.pair(u, raw, raw, 0)):
        with pytest.raises(api.LvfError) as e:
            call()
        assert "lvf error 1:" in str(e.value) and len(str(e.value)) > 20
    ctx2 = api.Context(0)
    foreign = api.Undistort(ctx2, cam, uc.BARREL, w, h)
    with pytest.raises(api.LvfError) as e:
        u.pair(foreign, raw, raw, 0)
    assert "different contexts" in str(e.value)
    foreign.close(); ctx2.close()
    # the objects stay usable
    img = u.image(raw, 0)
    assert np.array_equal(img.level(0)[0], ur.undistort(raw, cam, uc.BARREL))
    img.close(); u.close(); other.close()
