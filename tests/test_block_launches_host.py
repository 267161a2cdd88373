"""The launch stream of the MMDiT blocks, pinned on the host: for every mode of tests/block_launch_recorder.py (the four precision levels
with and without e4m3 attention, both IP-Adapter forms, injected samples, given adaLN vectors, the row window, the unfused q/k pass, a
width the fused q/k epilogue does not cover) plan_double + plan_single + run_double + run_single must make exactly the native calls,
with exactly the arguments, that tests/golden/block_launches.json holds. The fixture was recorded once from the tree in which every
projection was still written out per level, and names buffers by parameter name or order of appearance only, so it holds for any
layout of the plans and the workspace."""
import json

import pytest

import block_launch_recorder as blr


@pytest.fixture(scope="module")
def golden():
    with open(blr.FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_exactly_the_recorded_modes(golden):
    assert sorted(golden) == sorted(blr.MODES)
    # a bf16 double block makes 9 native calls, a single block 5; 2 + 1 of them the on-the-fly adaLN GEMVs
    assert len(golden["bf16"]) == 9 + 5 and sum(line.startswith("rt_gemv_bf16w(") for line in golden["bf16"]) == 3


@pytest.mark.parametrize("mode", list(blr.MODES))
def test_launch_stream_is_the_recorded_one(golden, mode):
    got, want = blr.record(**blr.MODES[mode]), golden[mode]
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            pytest.fail(f"{mode}: launch {i} differs\n  recorded: {w}\n  now:      {g}", pytrace=False)
    assert len(got) == len(want), f"{mode}: {len(got)} launches, recorded {len(want)}; first extra or missing: {(got + want)[min(len(got), len(want))]}"


@pytest.mark.parametrize("H,raises", [(1, True), (2, False)])
def test_mx_level_refuses_a_width_that_is_no_multiple_of_256(H, raises):
    from reptext_amd import mmdit

    for plan, blk in zip((mmdit.plan_double, mmdit.plan_single), blr.blocks(H)):
        rec = blr.Recorder()
        rec.blocks = {"block": blk}
        with blr.recording(rec):
            if raises:
                with pytest.raises(ValueError, match="the 'mx' level needs an inner width that is a multiple of 256"):
                    plan(blk, fp8="mx")
            else:
                plan(blk, fp8="mx")
