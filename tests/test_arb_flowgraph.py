"""Run tests/cpp/qa_arb.cpp (built by `make tests`): pfb_arb_resampler_ccf through the runtime.
ArbCpu.* is the CPU block on scheduler_mt against an in-test double reference (output count, buffer
sizes, advancing calls at r = 1/64, restart and time shard, the tone at f / r_eff); ArbHip.* the GPU
block in a scheduler_hip domain against the CPU block, restarted twice, and its time shard."""
import pytest

from tests.test_cpp_runtime import run


def test_arb_cpu_block():
    out = run("qa_arb", 300, "ArbCpu")
    assert "10 test(s), 0 failure(s)" in out


@pytest.mark.gpu
def test_arb_hip_block():
    out = run("qa_arb", 600, "ArbHip")
    print(out)
    assert "5 test(s), 0 failure(s)" in out
