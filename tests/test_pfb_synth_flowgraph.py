"""Run tests/cpp/qa_pfb_synth.cpp (built by `make tests`): pfb_synthesizer_ccf through the runtime.
PfbSynthCpu.* is the CPU block on scheduler_mt against an in-test double reference; PfbSynthHip.* the
GPU block in a scheduler_hip domain against the CPU block, a time shard, the scheduler's kernel
timing and the round trip hip::pfb_synthesizer_ccf -> hip::pfb_channelizer_ccf over a device edge."""
import pytest

from tests.test_cpp_runtime import run


def test_pfb_synth_cpu_block():
    out = run("qa_pfb_synth", 300, "PfbSynthCpu")
    assert "5 test(s), 0 failure(s)" in out


@pytest.mark.gpu
def test_pfb_synth_hip_block():
    out = run("qa_pfb_synth", 600, "PfbSynthHip")
    assert "7 test(s), 0 failure(s)" in out
