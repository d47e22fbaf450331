"""Host-side sanitizer run of csrc/conv_f32.hip's pure-host exports (``iit_conv_f32_ok``, ``iit_conv_f32_plan``): a
stand-alone program (tests/native/conv_f32_host.cpp) built with AddressSanitizer on the host half
(``-Xarch_host -fsanitize=address``) and executed on the CPU, as tests/test_native_host.py does for the other kernels.
Nothing is preloaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_conv_f32_host_checks_under_asan(tmp_path):
    exe = str(tmp_path / "conv_f32_host")
    src = [os.path.join(ROOT, "tests", "native", "conv_f32_host.cpp"), os.path.join(ROOT, "csrc", "conv_f32.hip")]
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "csrc"),
           "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fno-omit-frame-pointer", "-o", exe] + src
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "conv_f32 host checks passed" in run.stdout
