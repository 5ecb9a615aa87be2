"""Run tests/cpp/qa_resamp.cpp (built by `make tests`): rational_resampler_ccf through the runtime.
ResampCpu.* is the CPU block on scheduler_mt against an in-test double reference; ResampHip.* the GPU
block in a scheduler_hip domain against the CPU block."""
import pytest

from tests.test_cpp_runtime import run


def test_resamp_cpu_block():
    out = run("qa_resamp", 300, "ResampCpu")
    assert "7 test(s), 0 failure(s)" in out


@pytest.mark.gpu
def test_resamp_hip_block():
    out = run("qa_resamp", 600, "ResampHip")
    assert "6 test(s), 0 failure(s)" in out
