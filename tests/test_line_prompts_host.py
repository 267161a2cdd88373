"""Host side of per-line prompts: the known answers of ``pipeline.line_prompt_groups`` (the visibility contract), the refusals of
``line_prompt_arguments`` by argument name and before any native call, and the record that carries the three keywords. No kernel runs."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_true_cfg_host import _kw, _pipe, assert_no_call_state, no_native_call  # noqa: E402,F401

MASKS = [torch.tensor([1.0, 0.0, 0.5, 0.0]), torch.tensor([0.0, 0.0, 1.0, 0.0])]


def rows(table):
    return table.numpy().view(np.uint32)


def test_known_answers_of_the_visibility_contract():
    from reptext_amd.pipeline import line_prompt_groups

    ends, vis = line_prompt_groups(64, 64, MASKS, 4)
    assert ends == (64, 128, 192, 196)
    assert vis.dtype == torch.int32 and vis.shape == (1, 196)
    v = rows(vis)[0]
    assert (v[:64] == 9).all()                       # base text rows: {0, 3}
    assert (v[64:128] == 10).all()                   # line 1: {1, 3}
    assert (v[128:192] == 12).all()                  # line 2: {2, 3}
    assert v[192:].tolist() == [11, 9, 15, 9]        # image rows: {0, 3} + the lines whose mask is > 0 there; overlapping boxes OR
    # true CFG: [negative, positive]; the negative half's image rows see {0, 3} only, its text rows what the positive half's see
    ends2, vis2 = line_prompt_groups(64, 64, MASKS, 4, cfg=True)
    v2 = rows(vis2)
    assert ends2 == ends and v2.shape == (2, 196)
    assert (v2[1] == v).all() and (v2[0, :192] == v[:192]).all() and v2[0, 192:].tolist() == [9, 9, 9, 9]
    # the [1, N, 1] and per-image [B, N, 1] forms of the masks
    per_image = [torch.stack([MASKS[0], MASKS[1]]).reshape(2, 4, 1), MASKS[1].reshape(1, 4, 1)]
    _, vis3 = line_prompt_groups(64, 64, per_image, 4, batch=2, cfg=True)
    v3 = rows(vis3)
    assert v3.shape == (4, 196) and v3[2, 192:].tolist() == [11, 9, 15, 9] and v3[3, 192:].tolist() == [9, 9, 15, 9]
    assert (v3[:2, 192:] == 9).all()


def test_a_none_entry_creates_no_group():
    from reptext_amd.pipeline import line_prompt_groups

    ends, vis = line_prompt_groups(64, 128, MASKS, 4, has_prompt=[False, True])
    assert ends == (64, 192, 196)
    v = rows(vis)[0]
    assert (v[:64] == 5).all() and (v[64:192] == 6).all() and v[192:].tolist() == [5, 5, 7, 5]     # the second line's mask, bit 1
    assert line_prompt_groups(64, 64, MASKS, 4, has_prompt=[False, False]) is None
    with pytest.raises(ValueError, match="multiples of 64"):
        line_prompt_groups(60, 64, MASKS, 4)
    with pytest.raises(ValueError, match="at most 30"):
        line_prompt_groups(64, 64, [MASKS[0]] * 31, 4)
    ends31, vis31 = line_prompt_groups(64, 64, [MASKS[0]] * 30, 4)
    assert len(ends31) == 32 and int(rows(vis31)[0, -4]) == 0xFFFFFFFF and int(rows(vis31)[0, -1]) == (1 | 1 << 31)


def test_the_argument_errors(no_native_call):
    from reptext_amd.pipeline import LineCallExtensions, line_prompt_arguments

    masks = ["m0", "m1"]
    ok = LineCallExtensions(control_prompt=["a red neon sign", None])
    assert line_prompt_arguments(ok, 2, masks) == ["a red neon sign", None]
    assert line_prompt_arguments(LineCallExtensions(), 2, masks) is None
    assert line_prompt_arguments(LineCallExtensions(control_prompt=[None, None]), 2, None) is None
    e = torch.zeros(1, 128, 64)
    assert line_prompt_arguments(LineCallExtensions(control_prompt_embeds=[e, None]), 2, masks)[0] is e
    for ext, n_lines, m, fp8, match in (
            (LineCallExtensions(control_prompt=["a"]), 2, masks, False, "one entry per text line"),
            (LineCallExtensions(control_prompt="a"), 1, masks[:1], False, "one entry per text line"),
            (LineCallExtensions(control_prompt=["a", 7]), 2, masks, False, "string or None"),
            (LineCallExtensions(control_prompt=["a", "b"], control_prompt_max_sequence_length=100), 2, masks, False, "multiple of 64"),
            (LineCallExtensions(control_prompt=["a", "b"], control_prompt_max_sequence_length=576), 2, masks, False, "at most 512"),
            (LineCallExtensions(control_prompt=["a", "b"]), 2, None, False, "control_mask"),
            (LineCallExtensions(control_prompt=["a"] * 31), 31, ["m"] * 31, False, "at most 30"),
            (LineCallExtensions(control_prompt=["a", "b"], control_prompt_embeds=[e, e]), 2, masks, False, "not both"),
            (LineCallExtensions(control_prompt_embeds=[torch.zeros(1, 64, 64), None]), 2, masks, False, "control_prompt_max_sequence_length"),
            (LineCallExtensions(control_prompt=["a", "b"]), 2, masks, True, "enable_fp8_attention")):
        with pytest.raises(ValueError, match=match):
            line_prompt_arguments(ext, n_lines, m, fp8)


def test_the_pipelines_refuse_before_any_kernel(no_native_call):
    pipe = _pipe()
    hint = [torch.zeros(1, 16, 128)]
    with pytest.raises(ValueError, match="control_mask"):
        pipe(**_kw(), control_image=hint, control_prompt=["white chalk on a blackboard"])
    with pytest.raises(ValueError, match="one entry per text line"):
        pipe(**_kw(), control_image=hint, control_prompt=["a", "b"], control_mask=[torch.zeros(1, 16, 1)])
    pipe.transformer._fp8_attention = True
    with pytest.raises(ValueError, match="enable_fp8_attention"):
        pipe(**_kw(), control_image=hint, control_prompt_embeds=[torch.zeros(1, 128, 64)], control_mask=[torch.zeros(1, 16, 1)])
    assert_no_call_state(pipe)
    with pytest.raises(ValueError, match="inpaint pipeline does not support per-line prompts"):
        _pipe(inpaint=True)(**_kw(), control_prompt=["a"])


def test_the_record_carries_the_new_fields():
    from reptext_amd import pipeline
    from reptext_amd.pipeline import CallExtensions, LineCallExtensions, LoopExtras

    names = [f.name for f in dataclasses.fields(LineCallExtensions)]
    assert tuple(names[-3:]) == pipeline.LINE_PROMPT_ARGUMENTS == ("control_prompt", "control_prompt_embeds", "control_prompt_max_sequence_length")
    assert names[:-3] == [f.name for f in dataclasses.fields(CallExtensions)] and issubclass(LineCallExtensions, CallExtensions)
    d = LineCallExtensions()
    assert d.control_prompt is None and d.control_prompt_embeds is None and d.control_prompt_max_sequence_length == 128
    assert "line_prompts" in {f.name for f in dataclasses.fields(LoopExtras)} and LoopExtras().line_prompts is None
    # a call that names one of them carries the wider record for its duration, any other call the plain one
    pipe = _pipe()
    seen = []
    pipe.check_inputs = lambda *a, **k: seen.append(pipe._call_extensions)
    for kw in (dict(control_prompt=["x"], true_cfg_scale=2.0), dict(true_cfg_scale=2.0)):
        with pytest.raises(Exception):
            pipe(**dict(_kw(), prompt_embeds=None), **kw)
    assert seen == [LineCallExtensions(control_prompt=["x"], true_cfg_scale=2.0), CallExtensions(true_cfg_scale=2.0)]
    assert type(seen[1]) is CallExtensions and pipe._call_extensions is None
