"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol include/lvf.h declares,
and refuses to run without a GPU (no silent CPU fallback)."""
import ctypes as C
import os

import pytest

from lvio_fusion_amd import _lib


@pytest.fixture(scope="module")
def so():
    _lib.build()
    return C.CDLL(_lib.SO_PATH)


def test_every_declared_symbol_is_exported(so):
    names = _lib.declared_symbols()
    assert len(names) >= 40
    missing = [n for n in names if not hasattr(so, n)]
    assert not missing, f"declared in include/lvf.h but not exported: {missing}"
    # and the ctypes signature table covers the header
    assert sorted(_lib._SIGS) == names


def test_struct_layouts_match_header():
    assert C.sizeof(_lib.Camera) == 11 * 8
    assert C.sizeof(_lib.SolverOptions) == 8 * 8
    assert C.sizeof(_lib.IcpOptions) == 40


def test_no_cpu_fallback_without_gpu():
    # asked in a child process: torch brings its own copy of the HIP runtime, and initialising that copy in this process after the library
    # has loaded the system one leaves the library's runtime without a device for every later test of the session
    import subprocess
    import sys
    probe = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], capture_output=True, text=True, timeout=600, check=True)
    if probe.stdout.strip().splitlines()[-1] == "True":
        pytest.skip("GPU present")
    from lvio_fusion_amd import api
    with pytest.raises(api.LvfError) as e:
        api.Context(0)
    assert "no usable HIP device" in str(e.value) or "HIP error" in str(e.value)


def test_product_path_does_not_touch_oracle():
    """Nothing under lvio_fusion_amd/ or include/ may import, include or link the oracle."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for sub in ("lvio_fusion_amd", "include"):
        for dp, _, fs in os.walk(os.path.join(root, sub)):
            for f in fs:
                if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp", ".sh")):
                    txt = open(os.path.join(dp, f), errors="ignore").read()
                    for needle in ("pyoracle", "liblvf_oracle", "oracle/", "import oracle", "from oracle"):
                        hits = [ln for ln in txt.splitlines() if needle in ln and not ln.lstrip().startswith(("//", "#", "*", '"""'))]
                        # comments may cite the oracle; code may not use it
                        code_hits = [ln for ln in hits if "oracle/se3_ops.h" not in ln and "oracle/imu.h" not in ln and "oracle's" not in ln]
                        assert not code_hits, f"{sub}/{f} references the oracle: {code_hits[:2]}"


def test_recorded_window_equals_walk_host_only(tmp_path):
    """The host half of the Ceres surface, no GPU involved: adapt::Problem's recorder (payload captured while BuildProblem adds blocks,
    lvf_ceres_adapter.hpp gpu::Recorder) must assemble exactly the window the walk over the finished ceres::Problem builds — every SoA
    array, the keyframe / landmark numbering, weights, cameras, the Huber width, pose priors and the constant-pose mask."""
    import json
    import subprocess
    import numpy as np
    from lvio_fusion_amd import synthetic as syn
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "lvio_fusion_amd", "host", "adapter_selftest")
    if not os.path.exists(exe):
        pytest.skip("adapter_selftest not built (run __graft_entry__.build())")
    dump = lambda d, name, a, dt: np.ascontiguousarray(a, dtype=dt).tofile(os.path.join(d, name))
    camv = lambda c: np.concatenate([[c["fx"], c["fy"], c["cx"], c["cy"]], c["extrinsic"]])
    for case, (with_imu, weak_thr, const_kf) in enumerate(((True, 0, 0), (False, 10 ** 6, -1))):
        cfg = syn.config4_window(n_kf=9, n_lm=250, n_prewindow=50, seed=31 + case, imu_samples=3)
        tc = cfg["tc"]; o = np.argsort(tc["kf_idx"], kind="stable"); tc = {k: v[o] for k, v in tc.items()}
        tf, po = cfg["tf"], cfg["po"]
        d = str(tmp_path / f"c{case}"); os.makedirs(d)
        dump(d, "meta.i32", [cfg["n_kf"], cfg["n_lm"], 1, weak_thr, const_kf], np.int32)
        for name in ("poses", "vel", "ba", "bg", "inv_depth", "w_kf"):
            dump(d, name + ".f64", cfg[name], np.float64)
        dump(d, "cam0.f64", camv(cfg["cam0"]), np.float64); dump(d, "cam1.f64", camv(cfg["cam1"]), np.float64)
        dump(d, "tc_left_ob.f64", tc["left_ob"], np.float64); dump(d, "tc_right_ob.f64", tc["right_ob"], np.float64)
        dump(d, "tc_lm.i32", tc["lm_idx"], np.int32); dump(d, "tc_kf.i32", tc["kf_idx"], np.int32)
        dump(d, "tf_first_ob.f64", tf["first_ob"], np.float64); dump(d, "tf_ob.f64", tf["ob"], np.float64)
        dump(d, "tf_lm.i32", tf["lm_idx"], np.int32); dump(d, "tf_kf1.i32", tf["kf1_idx"], np.int32); dump(d, "tf_kf2.i32", tf["kf2_idx"], np.int32)
        dump(d, "po_ob.f64", po["ob"], np.float64); dump(d, "po_pw.f64", po["pw"], np.float64)
        dump(d, "po_kf.i32", po["kf_idx"], np.int32); dump(d, "po_pw_idx.i32", po["pw_idx"], np.int32)
        imu = cfg["imu"] if with_imu else []
        dump(d, "preint.f64", np.random.default_rng(case).normal(0, 1, (len(imu), 467)), np.float64)      # (content is payload only: copied, never evaluated here)
        dump(d, "imu_i.i32", [f["kf_i"] for f in imu], np.int32); dump(d, "imu_j.i32", [f["kf_j"] for f in imu], np.int32)
        env = dict(os.environ); env["LVF_SELFTEST_HOSTONLY"] = "1"
        p = subprocess.run([exe, "window", d], capture_output=True, text=True, timeout=120, env=env)
        assert p.returncode == 0, p.stdout + p.stderr
        out = json.loads(p.stdout.strip().splitlines()[-1])
        assert out["walk_ok"] == 1 and out["recorder_usable"] == 1 and out["recorded_equals_walk"] == 1, out
        assert out["n_kf"] == cfg["n_kf"] and out["blocks"] >= len(tf["lm_idx"]) + len(tc["lm_idx"])
        assert (out["n_prior"] > 0) == (not with_imu)


def test_host_alloc_works_without_a_device():
    """lvf_host_alloc hands out page-locked memory on a GPU box and ordinary memory elsewhere (host-only tools): usable, 64-byte aligned,
    and lvf_host_free takes it back either way; a pointer that is not ours is left alone."""
    import ctypes as C
    from lvio_fusion_amd import _lib
    L = _lib.lib()
    blocks = []
    for n in (1, 4096, 300000):
        p = L.lvf_host_alloc(n)
        assert p and p % 64 == 0
        C.memset(p, 0xAB, n)
        assert (C.c_ubyte * n).from_address(p)[n - 1] == 0xAB
        blocks.append((p, n))
    for p, n in blocks:
        L.lvf_host_free(p, n)
    L.lvf_host_free(None, 0)


def test_compiled_dropin_loads_and_links_the_hip_library():
    """oracle/_ref/liblvf_dropin.so (the reference's backend.cpp / association.cpp compiled unmodified against include/reference_patch): it loads,
    exports its two entry points and takes every lvf_* symbol it needs from liblvf_hip.so — no compute without a GPU"""
    import ctypes
    import subprocess
    import pytest
    from oracle import pydropin
    if not pydropin.available():
        pytest.skip("needs /root/reference at build time")
    from lvio_fusion_amd import _lib
    _lib.build(force=False)               # the drop-in links liblvf_hip.so: make sure it exists before `make dropin`
    so = pydropin.build()
    lib = ctypes.CDLL(so)
    for name in ("lvd_backend_solve", "lvd_scan_to_map_solve", "lvd_sources"):
        getattr(lib, name)
    nm = subprocess.run(["nm", "-D", "--undefined-only", so], capture_output=True, text=True).stdout
    needed = sorted({l.split()[-1] for l in nm.splitlines() if " lvf_" in l})
    assert "lvf_problem_solve" in needed or any(n.startswith("lvf_problem") for n in needed)
    declared = set(_lib.declared_symbols())
    assert set(needed) <= declared, sorted(set(needed) - declared)
    # the reference's factories resolve to the library's cost functions: no Jet-differentiated TwoFrame / PoseOnly functor is instantiated
    syms = subprocess.run(["nm", "-DC", so], capture_output=True, text=True).stdout
    assert "gpu::TwoFrameReprojectionError" in syms and "AutoDiffCostFunction<lvio_fusion::TwoFrameReprojectionError" not in syms
