"""Run tests/cpp/qa_psd.cpp (built by `make tests`): psd_vcf through the runtime. PsdCpu.* is the CPU
block on scheduler_mt against an in-test double computation (input counts that are no multiple of navg,
dB) and the refusals of both blocks' constructors; PsdHip.* the GPU block in a scheduler_hip domain
against the double computation and the CPU block at (N, K) = (64, 5), (1024, 16), (4096, 100), work()
calls that are no multiples of K, a restart, dB, and the block's kernel timing."""
import pytest

from tests.test_cpp_runtime import run


def test_psd_cpu_block():
    out = run("qa_psd", 300, "PsdCpu")
    assert "5 test(s), 0 failure(s)" in out


@pytest.mark.gpu
def test_psd_hip_block():
    out = run("qa_psd", 600, "PsdHip")
    assert "5 test(s), 0 failure(s)" in out
