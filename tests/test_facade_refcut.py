"""Row (b), on the reference's own text. oracle/ref/build_refcut.py cuts the reference's CALL SITES of the hot path -- the estimator's OpenMP front end
(estimator.cpp:248-270), kdtree_*_from_map->setInputCloud (lidar_mapper_keyframe.cpp:433-434), the AddResidualBlock loops (cpp:537-571) -- and the reference's own
TYPES (pcl::PointXYZIWithCov, common::PointICloud, cloudFeature, PointPlaneFeature, ScanInfo, Pose) out of /root/reference and compiles them, unchanged, against
m-loam_amd/host/mloam_facade.hpp in its in-tree mode (-DMLOAM_FACADE_USE_PCL_TYPES -DMLOAM_FACADE_CERES_BASES) over headers shaped like PCL / boost / Eigen / Ceres
(tests/host/pcl_stub). Here (no GPU): that it compiles; that the build-system stub INTEGRATION.md section 1 shows compiles as printed; and the host-only part run --
the residual blocks the reference's loops create from the facade's factor classes, owned by ceres::Problem, evaluated through the interface Ceres calls, against the
reference's own factor classes (oracle/_ref). The GPU legs are in tests/test_gpu_facade.py."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _refcut():
    spec = importlib.util.spec_from_file_location("build_refcut", os.path.join(ROOT, "oracle", "ref", "build_refcut.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _need_lib():
    if not os.path.exists(os.path.join(ROOT, "m-loam_amd", "lib", "libmloam_hip.so")):
        pytest.skip("libmloam_hip.so not built")


def test_reference_call_sites_compile_against_the_facade():
    """the three cut call sites + the reference's own types compile VERBATIM; a drifted reference tree or a facade that stops accepting them fails here"""
    _need_lib()
    rc = _refcut()
    if not os.path.isdir(os.path.join(rc.REF, "estimator", "src")):
        pytest.skip("no reference tree on this box (the prebuilt executable is exercised by the GPU test)")
    exe = rc.build(force=True)
    assert exe and os.path.exists(exe)
    assert not os.path.exists(rc.GEN), "cut reference text must not outlive the compile"


def test_add_residual_block_loops_own_the_facades_factors(tmp_path, orc):
    """lidar_mapper_keyframe.cpp:537-571, the reference's lines, on 2 000 random features: `new LidarMapPlaneNormFactor(feature.point_, feature.coeffs_, cov_matrix)`
    with Eigen arguments resolves to the facade's class, which IS a ceres::SizedCostFunction<1, 7>; problem.AddResidualBlock takes ownership (every allocation gone
    with the Problem); each block evaluated through CostFunction::Evaluate == the reference's own factor class (oracle/_ref), with_ua_flag on (extractCov of the
    feature's point) and off (COV_MEASUREMENT)."""
    _need_lib()
    if orc.ref_lib() is None:
        pytest.skip("no reference build")
    exe = _refcut().build()
    if exe is None:
        pytest.skip("no reference tree and no prebuilt refcut_selftest")
    rng = np.random.default_rng(77)
    n = 2000
    rows = np.zeros((n, 26))
    for i in range(n):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        pose = np.concatenate([rng.uniform(-30, 30, 3), q])
        sd = rng.uniform(0.01, 0.6, 3)
        cov = np.diag(sd ** 2); cov[0, 1] = cov[1, 0] = 0.1 * sd[0] * sd[1]
        cov = cov.astype(np.float32).astype(np.float64)            # the covariance travels in the feature's float fields (point_with_cov.hpp:90-100)
        kind = i % 2
        if kind == 0:
            nrm = rng.normal(size=3); nrm /= np.linalg.norm(nrm)
            coeff = np.concatenate([nrm, [rng.uniform(-5, 5)], [0, 0]])
        else:
            c = rng.uniform(-40, 40, 3); v = rng.normal(size=3); v /= np.linalg.norm(v)
            coeff = np.concatenate([c + 0.1 * v, c - 0.1 * v])
        rows[i] = np.concatenate([[kind], rng.uniform(-40, 40, 3), coeff, cov.ravel(), pose])
    rows.tofile(tmp_path / "factors.f64")
    r = subprocess.run([exe, "cpu", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "owned and released by ceres::Problem: yes" in r.stdout
    out = np.fromfile(tmp_path / "factors_out.f64").reshape(2, n, 8)
    cov_meas = np.diag([0.0025] * 3)
    for ua in (0, 1):
        for i in range(n):
            kind = "s" if rows[i, 0] == 0 else "c"
            # with_ua_flag: extractCov reads the six floats back into a SYMMETRIC matrix (point_with_cov.hpp:202-214); only its trace enters the weight
            cov = rows[i, 10:19].reshape(3, 3) if ua else cov_meas
            r_ref, J_ref = orc.ref_map_factor(kind, rows[i, 1:4], rows[i, 4:10][: 4 if kind == "s" else 6], cov, rows[i, 19:26])
            assert abs(out[ua, i, 0] - r_ref) <= 1e-12 * max(1.0, abs(r_ref)), (ua, i, kind)
            np.testing.assert_allclose(out[ua, i, 1:], J_ref, rtol=1e-11, atol=1e-11)


def test_integration_section_1_compiles_as_printed(tmp_path):
    """INTEGRATION.md section 1 shows the translation-unit preamble a maintainer adds inside the reference tree. The fenced block tagged `integration-section-1` is
    extracted from the document and compiled as it stands against the PCL / Eigen / Ceres-shaped stubs: if the facade's in-tree mode or the document drift apart,
    this fails (the round-4 text did not compile -- PointXYZ was missing from its alias list)."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"<!-- integration-section-1 -->\s*```cpp\n(.*?)```", text, re.S)
    assert m, "INTEGRATION.md lost its tagged section-1 snippet"
    src = tmp_path / "integration_section_1.cpp"
    src.write_text(m.group(1))
    rc = _refcut()
    # (the reference's own mloam_pcl/point_with_cov.hpp is on the include path inside its tree; here a stand-in with that header's layout)
    cmd = [c for c in rc.compile_cmd(str(tmp_path / "snippet.o"), str(src), extra=("-I", os.path.join(ROOT, "tests", "host", "pcl_stub_mloam")))
           if not c.startswith("-l") and not c.startswith("-L") and not c.startswith("-Wl,")]
    cmd.insert(1, "-c")
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
