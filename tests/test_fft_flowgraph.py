"""Run tests/cpp/qa_fft.cpp (built by `make tests`): fft_vcc through the runtime. FftCpu.* is the CPU
block on scheduler_mt against an in-test O(N^2) double DFT, its own round trip and the refusals of
both blocks; FftHip.* the GPU block in a scheduler_hip domain against the CPU block at four sizes,
the channelizer fusion (taken only at 1024 points without window and shift) and the scheduler's
kernel timing."""
import pytest

from tests.test_cpp_runtime import run


def test_fft_cpu_block():
    out = run("qa_fft", 300, "FftCpu")
    assert "4 test(s), 0 failure(s)" in out


@pytest.mark.gpu
def test_fft_hip_block():
    out = run("qa_fft", 600, "FftHip")
    assert "9 test(s), 0 failure(s)" in out
