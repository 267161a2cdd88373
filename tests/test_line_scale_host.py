"""Host side of a strength per line prompt (``control_prompt_scale``): the known answers of ``pipeline.line_prompt_bias`` (the rule: ln w_r
on key class r), written out by hand; every refusal; the record that carries the keyword and the one that carries the table; the
graph key; the launch stream of one double and one single block with ``key_bias`` against the same blocks without; and the argument
checks of ``ops.attention`` that need no device memory. No kernel runs."""
import ctypes as C
import dataclasses
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_true_cfg_host import _kw, _pipe, assert_no_call_state, no_native_call  # noqa: E402,F401

f32 = lambda x: float(np.float32(x))


def test_known_answers_of_the_rule():
    from reptext_amd.pipeline import line_prompt_bias

    t = line_prompt_bias([2.0, 0.5], [True, True])
    assert t.dtype == torch.float32 and t.shape == (1, 32) and t.is_contiguous()
    assert t[0, 1].item() == f32(math.log(2.0)) == f32(0.6931471805599453) and t[0, 2].item() == f32(-0.6931471805599453)
    assert t[0, 0].item() == 0.0 and not t[0, 3:].any()                              # the base prompt and every image class: no bias
    # a line without a prompt does not consume an index: the third line's prompt is class 2
    t = line_prompt_bias([4.0, None, 0.25, 1.0], [True, False, True, False])
    assert t[0, 1].item() == f32(math.log(4.0)) and t[0, 2].item() == f32(math.log(0.25)) and not t[0, 3:].any() and t[0, 0].item() == 0.0
    # None is 1.0, which gives 0.0; so does the scale of a line without a prompt, whatever it is (the call refuses a non-unit one)
    t = line_prompt_bias([None, 3.0], [True, True])
    assert t[0, 1].item() == 0.0 and t[0, 2].item() == f32(1.0986122886681098)
    assert not line_prompt_bias([1.0, None], [True, True]).any() and not line_prompt_bias([None], [False]).any()
    # the ends of the stated range, to fp32
    t = line_prompt_bias([64.0, 1 / 64], [True, True])
    assert t[0, 1].item() == f32(4.1588830833596715) and t[0, 2].item() == f32(-4.1588830833596715)
    # 30 line prompts fill classes 1..30
    t = line_prompt_bias([2.0] * 30, [True] * 30)
    assert (t[0, 1:31] == f32(math.log(2.0))).all() and t[0, 0].item() == 0.0 and t[0, 31].item() == 0.0
    for bad in (0.0, -1.0, 1 / 65, 64.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match=r"\[1/64, 64\]"):
            line_prompt_bias([bad], [True])
    with pytest.raises(ValueError, match="2 entries for 1"):
        line_prompt_bias([1.0, 1.0], [True])
    with pytest.raises(ValueError, match="at most 30"):
        line_prompt_bias([1.0] * 31, [True] * 31)


def test_the_argument_and_its_refusals():
    from reptext_amd.pipeline import LineScaleCallExtensions as Ext, line_scale_argument

    assert line_scale_argument(Ext(), ["a"], 1) is None and line_scale_argument(object(), ["a"], 1) is None      # absent, or None: not named
    assert line_scale_argument(Ext(control_prompt_scale=None), None, 1) is None
    assert line_scale_argument(Ext(control_prompt_scale=2), ["a", None, "b"], 3) == [2.0, 1.0, 2.0]            # a float: every line PROMPT
    assert line_scale_argument(Ext(control_prompt_scale=[2.0, None, 0.5]), ["a", None, "b"], 3) == [2.0, 1.0, 0.5]
    assert line_scale_argument(Ext(control_prompt_scale=(None, 1.0, None)), ["a", None, "b"], 3) == [1.0, 1.0, 1.0]
    assert line_scale_argument(Ext(control_prompt_scale=[1 / 64, 64]), ["a", "b"], 2) == [1 / 64, 64.0]
    with pytest.raises(ValueError, match="needs a per-line prompt"):
        line_scale_argument(Ext(control_prompt_scale=2.0), None, 1)
    for bad in ([2.0], [2.0, 1.0, 1.0], "2.0", [2.0, "1.0"], True, [True, 1.0], torch.ones(2)):
        with pytest.raises(ValueError, match="a float or a list with a float or None per text line"):
            line_scale_argument(Ext(control_prompt_scale=bad), ["a", "b"], 2)
    with pytest.raises(ValueError, match="without a prompt cannot have a scale"):
        line_scale_argument(Ext(control_prompt_scale=[2.0, 2.0]), ["a", None], 2)
    for bad in (0.0, -2.0, 1 / 65, 65.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match=r"finite and lies in \[1/64, 64\]"):
            line_scale_argument(Ext(control_prompt_scale=bad), ["a"], 1)
        with pytest.raises(ValueError, match=r"finite and lies in \[1/64, 64\]"):
            line_scale_argument(Ext(control_prompt_scale=[1.0, bad]), ["a", "b"], 2)


def test_the_refusals_of_a_call(no_native_call):
    pipe = _pipe()
    hint, mask = [torch.zeros(1, 16, 128)], [torch.zeros(1, 16, 1)]
    emb = [torch.zeros(1, 128, 64)]
    with pytest.raises(ValueError, match="control_prompt_scale needs a per-line prompt"):
        pipe(**_kw(), control_image=hint, control_mask=mask, control_prompt_scale=2.0)
    with pytest.raises(ValueError, match="control_prompt_scale needs a per-line prompt"):
        pipe(**_kw(), control_image=hint, control_mask=mask, control_prompt=[None], control_prompt_scale=[2.0])
    with pytest.raises(ValueError, match="per text line"):
        pipe(**_kw(), control_image=hint, control_mask=mask, control_prompt_embeds=emb, control_prompt_scale=[2.0, 1.0])
    with pytest.raises(ValueError, match=r"\[1/64, 64\]"):
        pipe(**_kw(), control_image=hint, control_mask=mask, control_prompt_embeds=emb, control_prompt_scale=100.0)
    with pytest.raises(ValueError, match=r"\[1/64, 64\]"):
        pipe(**_kw(), control_image=hint, control_mask=mask, control_prompt_embeds=emb, control_prompt_scale=[float("nan")])
    with pytest.raises(ValueError, match="without a prompt cannot have a scale"):
        pipe(**_kw(), control_image=hint * 2, control_mask=mask * 2, control_prompt_embeds=emb + [None], control_prompt_scale=[2.0, 0.5])
    with pytest.raises(ValueError, match="control_mask"):                    # what line_prompt_arguments refuses stays refused, and first
        pipe(**_kw(), control_image=hint, control_prompt=["white chalk"], control_prompt_scale=2.0)
    with pytest.raises(ValueError, match="not both"):
        pipe(**_kw(), control_image=hint, control_mask=mask, control_prompt=["x"], control_prompt_embeds=emb, control_prompt_scale=2.0)
    pipe.transformer._fp8_attention = True
    with pytest.raises(ValueError, match="enable_fp8_attention"):
        pipe(**_kw(), control_image=hint, control_prompt_embeds=emb, control_mask=mask, control_prompt_scale=2.0)
    assert_no_call_state(pipe)
    with pytest.raises(ValueError, match=r"inpaint pipeline does not support per-line prompts \(control_prompt_scale\)"):
        _pipe(inpaint=True)(**_kw(), control_prompt_scale=2.0)
    with pytest.raises(TypeError):                                           # still no such keyword as a misspelt one
        pipe(**_kw(), control_prompt_scales=2.0)


def test_the_records():
    from reptext_amd import pipeline
    from reptext_amd.pipeline import (CallExtensions, IsolatedLinePrompts, IsolationCallExtensions, LineCallExtensions, LinePrompts, LineScale,
                                      LineScaleCallExtensions, LoopExtras, RegionalIPCallExtensions)

    names = [f.name for f in dataclasses.fields(LineScaleCallExtensions)]
    assert tuple(names[-1:]) == pipeline.LINE_SCALE_ARGUMENTS == ("control_prompt_scale",) and LineScaleCallExtensions().control_prompt_scale is None
    assert names[:-1] == [f.name for f in dataclasses.fields(IsolationCallExtensions)] and issubclass(LineScaleCallExtensions, IsolationCallExtensions)
    assert pipeline.LINE_SCALE_RANGE == (1 / 64, 64.0)
    # the existing records are what they were
    assert names[-2] == "control_prompt_isolation" and len(dataclasses.fields(RegionalIPCallExtensions)) == 20
    assert len(dataclasses.fields(CallExtensions)) == 13 and len(dataclasses.fields(LineCallExtensions)) == 16
    assert [f.name for f in dataclasses.fields(LinePrompts)] == ["embeds", "ends", "row_vis"]
    assert [f.name for f in dataclasses.fields(IsolatedLinePrompts)] == ["embeds", "ends", "row_vis", "key_class"]
    assert LinePrompts.STATIC == {"line_embeds": "embeds", "line_row_vis": "row_vis"}
    assert IsolatedLinePrompts.STATIC == {"line_embeds": "embeds", "line_row_vis": "row_vis", "line_key_class": "key_class"}
    # only a call that names the keyword carries the new record
    pipe = _pipe()
    seen = []
    pipe.check_inputs = lambda *a, **k: seen.append(pipe._call_extensions)
    for kw in (dict(control_prompt=["x"], control_prompt_scale=[2.0]), dict(control_prompt=["x"], control_prompt_isolation=True),
               dict(control_prompt=["x"]), dict(control_prompt_scale=1.0), {}):
        with pytest.raises(Exception):
            pipe(**dict(_kw(), prompt_embeds=None), **kw)
    assert [type(s) for s in seen] == [LineScaleCallExtensions, IsolationCallExtensions, LineCallExtensions, LineScaleCallExtensions, CallExtensions]
    assert seen[0] == LineScaleCallExtensions(control_prompt=["x"], control_prompt_scale=[2.0]) and pipe._call_extensions is None
    # the table travels in a slot of its own, as one more static input; the line_prompts records and their keys are what they were
    emb, vis, kc = torch.zeros(2, 128, 48), torch.zeros(2, 208, dtype=torch.int32), torch.zeros(2, 208, dtype=torch.uint8)
    table = torch.zeros(1, 32)
    sig = lambda t: ("sig", tuple(t.shape), str(t.dtype))
    plain, iso, scale = LinePrompts(emb, (64, 192, 208), vis), IsolatedLinePrompts(emb, (64, 192, 208), vis, kc), LineScale(table)
    assert [f.name for f in dataclasses.fields(LineScale)] == ["key_bias"] and LineScale.STATIC == {"line_key_bias": "key_bias"}
    assert plain.signature(sig) == (("line_prompts", (64, 192, 208), sig(vis), sig(emb)),)
    assert iso.signature(sig) == plain.signature(sig) + (("line_isolation", sig(kc)),)
    assert scale.signature(sig) == (("line_scale", sig(table)),)
    assert LoopExtras().line_scale is None and [f.name for f in dataclasses.fields(LoopExtras)][-2:] == ["line_scale", "quiet"]
    for lp in (plain, iso):
        without, with_ = LoopExtras(line_prompts=lp), LoopExtras(line_prompts=lp, line_scale=scale)
        assert without.signature(sig, None, None) == lp.signature(sig)                                  # the key it had
        assert with_.signature(sig, None, None) == lp.signature(sig) + (("line_scale", sig(table)),)    # appended, last
        assert list(with_.tensors()) == list(without.tensors()) + ["line_key_bias"] and with_.tensors()["line_key_bias"] is table
        static = {k: t.clone() for k, t in with_.tensors().items()}
        bound = with_.rebound(static)
        assert type(bound.line_scale) is LineScale and bound.line_scale.key_bias is static["line_key_bias"] and type(bound.line_prompts) is type(lp)
        assert bound.signature(sig, None, None) == with_.signature(sig, None, None)
        assert without.rebound({k: t.clone() for k, t in without.tensors().items()}).line_scale is None
    # other VALUES of the scales give the same key: the table is a static input, its signature is its layout
    from reptext_amd.pipeline import line_prompt_bias
    key = lambda s: LoopExtras(line_prompts=plain, line_scale=LineScale(line_prompt_bias(s, [True, True]))).signature(sig, None, None)
    assert key([2.0, 0.5]) == key([1.0, 1.0]) == key([None, 64.0])


def _record(key_bias, keyed, H=2):
    """The launch stream of one double and one single block with key groups (or classes), with or without a bias table."""
    import block_launch_recorder as blr
    from reptext_amd import mmdit, ops

    class Rec(blr.Recorder):
        def pointer(self, ptr):
            return "host" if isinstance(ptr, C.c_void_p) else super().pointer(ptr)      # the group ends: a host array

    d, S = H * 128, blr.T + blr.N
    rec = Rec()
    with blr.recording(rec):
        dbl, sgl = blr.blocks(H)
        rec.blocks = {"double": dbl, "single": sgl}
        pd, ps = mmdit.plan_double(dbl), mmdit.plan_single(sgl)
        ws = mmdit.Workspace(blr.B, blr.T, blr.N, d, torch.device("cpu"), True)
        temb, cos, sin = rec.new(blr.B, d, dtype=blr.F32), rec.new(S, 128, dtype=blr.F32), rec.new(S, 128, dtype=blr.F32)
        vis = rec.track(torch.full((blr.B, S), 7, dtype=torch.int32))
        cls = rec.track(torch.zeros(blr.B, S, dtype=torch.uint8))
        bias = rec.track(torch.zeros(1, 32))
        assert [rec.pointer(t.data_ptr()) for t in (vis, cls, bias)] == ["b0+0", "b1+0", "b2+0"]       # named alike in every stream
        groups = ops.KeyClasses(vis, cls) if keyed else ops.KeyGroups((blr.T, S), vis)
        kw = dict(key_bias=bias) if key_bias else {}
        mmdit.run_double(pd, ws, temb, cos, sin, H, groups=groups, **kw)
        mmdit.run_single(ps, ws, temb, cos, sin, H, groups=groups, **kw)
    return rec.lines


@pytest.mark.parametrize("keyed", [False, True])
def test_the_launch_stream_differs_by_the_attention_entry_alone(keyed):
    """The same native calls in the same order on the same buffers; the two attention launches are the biased entry instead of the
    grouped (keyed) one, with the sibling's arguments unchanged and (table, 0) behind them: [1, 32], one table for the batch."""
    sibling = "rt_attention_fwd_keyed" if keyed else "rt_attention_fwd_grouped"
    plain, biased = _record(False, keyed), _record(True, keyed)
    name = lambda line: line.split("(", 1)[0]
    args = lambda line: line.split("(", 1)[1][:-1].split(", ")
    assert [name(x) for x in biased] == [name(x) + "_biased" if name(x) == sibling else name(x) for x in plain]
    assert sum(name(x) == sibling for x in plain) == 2 == sum(name(x) == sibling + "_biased" for x in biased)
    assert not any(name(x) == sibling for x in biased) and not any("biased" in x for x in plain)
    for p, b in zip(plain, biased):
        if name(p) != sibling:
            assert p == b
        else:
            assert args(b) == args(p) + ["b2+0", "0"]


def test_run_blocks_refuse_a_bias_without_groups():
    import block_launch_recorder as blr
    from reptext_amd import mmdit

    rec = blr.Recorder()
    with blr.recording(rec):
        dbl, sgl = blr.blocks(2)
        rec.blocks = {"double": dbl, "single": sgl}
        pd, ps = mmdit.plan_double(dbl), mmdit.plan_single(sgl)
        ws = mmdit.Workspace(blr.B, blr.T, blr.N, 256, torch.device("cpu"), True)
        temb, cos, sin = rec.new(blr.B, 256, dtype=blr.F32), rec.new(192, 128, dtype=blr.F32), rec.new(192, 128, dtype=blr.F32)
        with pytest.raises(ValueError, match="key_bias needs key groups"):
            mmdit.run_double(pd, ws, temb, cos, sin, 2, key_bias=torch.zeros(1, 32))
        with pytest.raises(ValueError, match="key_bias needs key groups"):
            mmdit.run_single(ps, ws, temb, cos, sin, 2, key_bias=torch.zeros(1, 32))


def test_the_op_refuses_before_any_native_call(no_native_call):
    """``ops.attention``'s checks of ``key_bias`` that need no device memory: they come before the pointers are taken."""
    from reptext_amd import ops

    B, S, H = 2, 128, 1
    buf = torch.zeros(B, S, 3 * 128, dtype=torch.bfloat16)
    q, k, v = buf[..., :128], buf[..., 128:256], buf[..., 256:]
    groups = ops.KeyGroups((64, 128), torch.zeros(1, S, dtype=torch.int32))
    keyed = ops.KeyClasses(torch.zeros(1, S, dtype=torch.int32), torch.zeros(1, S, dtype=torch.uint8))
    with pytest.raises(ValueError, match="key_bias= needs groups="):
        ops.attention(q, k, v, q, H, key_bias=torch.zeros(1, 32))
    with pytest.raises(ValueError, match="key_bias= needs groups="):
        ops.attention(q, k, v, q, H, rows=(0, 64), key_bias=torch.zeros(1, 32))
    from unittest import mock
    with mock.patch.object(torch.Tensor, "is_cuda", property(lambda self: True), create=True):      # past the row table's device check
        for g in (groups, keyed):
            for bad, exc, msg in ((torch.zeros(1, 32, dtype=torch.float64), TypeError, "float32"), (torch.zeros(1, 32, dtype=torch.bfloat16), TypeError, "float32"),
                                  ([0.0] * 32, TypeError, "float32"), (torch.zeros(32), ValueError, r"need \[2 or 1, 32\]"),
                                  (torch.zeros(3, 32), ValueError, r"need \[2 or 1, 32\]"), (torch.zeros(1, 31), ValueError, r"need \[2 or 1, 32\]"),
                                  (torch.zeros(2, 64)[:, ::2], ValueError, "unit inner stride"),
                                  (torch.zeros(1, 32, device="meta"), RuntimeError, "key_bias is on meta")):
                with pytest.raises(exc, match=msg):
                    ops.attention(q, k, v, q, H, groups=g, key_bias=bad)
