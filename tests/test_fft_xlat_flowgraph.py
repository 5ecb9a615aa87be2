"""Run tests/cpp/qa_fft_xlat.cpp (built by `make tests`): freq_xlating_fft_filter_ccc / _ccf through the
runtime. FftXlatCpu.* is the CPU block on scheduler_mt against an in-test double sum of the definition
and the refusals of both blocks' constructors; FftXlatHip.* the GPU blocks in a scheduler_hip domain
against the CPU block (complex and real taps at two (N, D), work() calls that are no multiples of the
frames' outputs), a restart from zero history, and a time shard with set_first_index."""
import pytest

from tests.test_cpp_runtime import run


def test_fft_xlat_cpu_block():
    out = run("qa_fft_xlat", 300, "FftXlatCpu")
    assert "4 test(s), 0 failure(s)" in out


@pytest.mark.gpu
def test_fft_xlat_hip_block():
    out = run("qa_fft_xlat", 600, "FftXlatHip")
    assert "5 test(s), 0 failure(s)" in out
