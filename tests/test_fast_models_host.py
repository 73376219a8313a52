"""The decided fast tier of the sgd / abc chains (csrc/djb_fast_models.inc) compiled FOR THE HOST (tools/sgd_fast_check.cpp: the same
source in its host-restated instantiation) against the host's glibc -- the reference's own pow / exp / acos -- and __float128:
no decided value may differ from the reference's float, and the measured distance must stay below the bound (the tool's exit code)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_tool(tmp_path):
    exe = str(tmp_path / "sgd_fast_check")
    cc = subprocess.run(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-fopenmp", "-I", os.path.join(ROOT, "dj_brdf_amd", "csrc"),
                         os.path.join(ROOT, "tools", "sgd_fast_check.cpp"), "-o", exe, "-lquadmath"], capture_output=True, text=True)
    if cc.returncode != 0 and "quadmath" in cc.stderr:
        pytest.skip("no libquadmath on this host")
    assert cc.returncode == 0, cc.stderr[-2000:]
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fast_tier_against_host_glibc(tmp_path):
    exe = _build_tool(tmp_path)
    r = subprocess.run([exe, os.path.join(ROOT, "dj_brdf_amd", "data", "sgd_params.csv"), "20000",
                        os.path.join(ROOT, "dj_brdf_amd", "data", "abc_params.csv"), "4000000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "MISMATCH" not in r.stdout
    for term in ("g1 :", "ndf:", "abc:"):
        line = [l for l in r.stdout.splitlines() if l.startswith(term)][0]
        assert " 0 decided-but-different" in line, line


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fast_tier_on_user_supplied_rows(tmp_path):
    """The same check over rows a caller can supply (tests/param_space_cases.py: every column resampled from the published values, and rows on
    and over every limit of the tier's domain): no decided value may differ from the reference's float.  alpha = 1e-12 is inside the domain
    and drives the ndf's relative bound above 1 (ax > 3.7e14): the lower end of the interval went negative, rounded to -0 and was "decided"
    against the upper end's +0 -- the reference returns +0.  (Only the counts are asserted: the tool's distance / bound figure also takes
    units whose exponent was clamped at -700, where both ends are +0 whatever the distance, so its exit code does not apply to these rows.)"""
    import param_space_cases as ps
    exe = _build_tool(tmp_path)
    data = os.path.join(ROOT, "dj_brdf_amd", "data")
    files = {}
    for kind, lead in (("sgd", ",,"), ("abc", ",")):
        rows = getattr(ps, kind + "_edge_rows")() + [("resampled %d" % k, r) for k, r in enumerate(ps.resampled_rows(kind))]
        files[kind] = str(tmp_path / (kind + "_rows.csv"))
        with open(os.path.join(data, kind + "_params.csv")) as f:
            header = f.readline()
        with open(files[kind], "w") as f:
            f.write(header)
            for name, row in rows:
                f.write(name.replace(",", ";") + lead + ",".join(repr(float(v)) for v in row) + "\n")
    r = subprocess.run([exe, files["sgd"], "400000", files["abc"], "1000"], capture_output=True, text=True, timeout=600)
    assert "MISMATCH" not in r.stdout, "\n".join(l for l in r.stdout.splitlines() if "MISMATCH" in l)[:3000]
    assert "alpha=1e-12" not in [l.split("(")[1].split(")")[0] for l in r.stdout.splitlines() if "outside the fast tier" in l]
    for term in ("g1 :", "ndf:", "abc:"):
        line = [l for l in r.stdout.splitlines() if l.startswith(term)][0]
        assert " 0 decided-but-different" in line, line
