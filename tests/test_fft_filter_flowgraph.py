"""Run tests/cpp/qa_fft_filter.cpp (built by `make tests`): fft_filter_ccc / fft_filter_ccf through the
runtime. FftFilterCpu.* is the CPU block on scheduler_mt against an in-test double convolution and the
refusals of both blocks' constructors; FftFilterHip.* the GPU blocks in a scheduler_hip domain against
the CPU block (complex and real taps, two frame sizes, work() calls that are no multiples of the valid
length), a restart from zero history, a time shard, and the scheduler's and the block's kernel timing."""
import pytest

from tests.test_cpp_runtime import run


def test_fft_filter_cpu_block():
    out = run("qa_fft_filter", 300, "FftFilterCpu")
    assert "4 test(s), 0 failure(s)" in out


@pytest.mark.gpu
def test_fft_filter_hip_block():
    out = run("qa_fft_filter", 600, "FftFilterHip")
    assert "6 test(s), 0 failure(s)" in out
