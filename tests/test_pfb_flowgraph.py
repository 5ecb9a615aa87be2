"""Run tests/cpp/qa_pfb.cpp (built by `make tests`): pfb_channelizer_ccf through the runtime.
PfbCpu.* is the CPU block on scheduler_mt against an in-test double reference; PfbHip.* the GPU block
in a scheduler_hip domain against the CPU block."""
import pytest

from tests.test_cpp_runtime import run


def test_pfb_cpu_block():
    out = run("qa_pfb", 300, "PfbCpu")
    assert "4 test(s), 0 failure(s)" in out


@pytest.mark.gpu
def test_pfb_hip_block():
    out = run("qa_pfb", 600, "PfbHip")
    assert "4 test(s), 0 failure(s)" in out
