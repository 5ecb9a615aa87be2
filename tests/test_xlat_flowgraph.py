"""Run tests/cpp/qa_xlat.cpp (built by `make tests`): rotator_cc and freq_xlating_fir_filter_ccf
through the runtime. XlatCpu.* are the CPU blocks on scheduler_mt against an in-test double
reference; XlatHip.* the GPU blocks in a scheduler_hip domain against the CPU blocks."""
import pytest

from tests.test_cpp_runtime import run


def test_xlat_cpu_blocks():
    out = run("qa_xlat", 300, "XlatCpu")
    assert "5 test(s), 0 failure(s)" in out


@pytest.mark.gpu
def test_xlat_hip_blocks():
    out = run("qa_xlat", 600, "XlatHip")
    assert "5 test(s), 0 failure(s)" in out
