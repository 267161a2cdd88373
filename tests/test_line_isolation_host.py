"""Host side of region isolation for per-line prompts (``control_prompt_isolation=True``): the known answers of
``pipeline.line_prompt_classes`` (the per-key visibility contract), written out by hand; the records that carry the keyword and the
class table; the refusals; and the launch stream of one double and one single block with ``ops.KeyClasses`` against the same blocks with
``ops.KeyGroups``. No kernel runs."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_true_cfg_host import _kw, _pipe, assert_no_call_state, no_native_call  # noqa: E402,F401

DISJOINT = [torch.tensor([1.0, 0.0, 0.0, 0.0]), torch.tensor([0.0, 0.0, 1.0, 0.0])]
OVERLAP = [torch.tensor([1.0, 0.0, 0.5, 0.0]), torch.tensor([0.0, 0.0, 1.0, 0.0])]


def words(table):
    return table.numpy().view(np.uint32)


def sees_a_key(row_vis, key_class):
    """Restated here: every row has the bit of at least one class that occurs among its entry's keys."""
    rv, kc = words(row_vis), key_class.numpy()
    return all(((rv[b][:, None] >> kc[b][None, :].astype(np.uint32)) & 1).any(axis=1).all() for b in range(rv.shape[0]))


def test_two_disjoint_boxes():
    from reptext_amd.pipeline import line_prompt_classes

    row_vis, key_class = line_prompt_classes(64, 64, DISJOINT, 4)
    assert row_vis.dtype == torch.int32 and key_class.dtype == torch.uint8 and row_vis.shape == key_class.shape == (1, 196)
    # classes: 0 base, 1 and 2 the lines, 3 the background, 4 = in box 1 only, 5 = in box 2 only
    kc, v = key_class[0].tolist(), words(row_vis)[0]
    assert kc[:64] == [0] * 64 and kc[64:128] == [1] * 64 and kc[128:192] == [2] * 64 and kc[192:] == [4, 3, 5, 3]
    assert (v[:64] == (1 | 8 | 16 | 32)).all()               # base text rows: the base prompt and every image class
    assert (v[64:128] == (2 | 16)).all()                     # line 1: itself and its own box
    assert (v[128:192] == (4 | 32)).all()                    # line 2
    # image rows: in box 1 -> base, line 1, background, box 1 (not box 2); outside -> base and every image class
    assert v[192:].tolist() == [1 | 2 | 8 | 16, 57, 1 | 4 | 8 | 32, 57]
    assert sees_a_key(row_vis, key_class)


def test_two_overlapping_boxes_get_an_overlap_class():
    from reptext_amd.pipeline import line_prompt_classes

    row_vis, key_class = line_prompt_classes(64, 64, OVERLAP, 4)
    # token 0 is in box 1 only, token 2 in both; "in box 2 only" does not occur and gets no class: 3 background, 4 = {1}, 5 = {1, 2}
    kc, v = key_class[0].tolist(), words(row_vis)[0]
    assert kc[192:] == [4, 3, 5, 3]
    assert (v[:64] == 57).all()
    assert (v[64:128] == (2 | 16 | 32)).all()                # line 1 reads box 1: the tokens in it alone and the overlap
    assert (v[128:192] == (4 | 32)).all()                    # line 2 reads box 2: only the overlap lies in it
    # token 0 ({1}): base, line 1, background, {1}, and {1, 2} (it intersects); token 2 ({1, 2}): both lines and everything that intersects
    assert v[192:].tolist() == [1 | 2 | 8 | 16 | 32, 57, 1 | 2 | 4 | 8 | 16 | 32, 57]
    assert sees_a_key(row_vis, key_class)


def test_a_line_without_a_prompt_creates_no_class():
    from reptext_amd.pipeline import line_prompt_classes

    row_vis, key_class = line_prompt_classes(64, 128, OVERLAP, 4, has_prompt=[False, True])
    kc, v = key_class[0].tolist(), words(row_vis)[0]
    assert row_vis.shape == (1, 64 + 128 + 4)
    assert kc[:64] == [0] * 64 and kc[64:192] == [1] * 128 and kc[192:] == [2, 2, 3, 2]        # 2 the background, 3 = in the second line's box
    assert (v[:64] == (1 | 4 | 8)).all() and (v[64:192] == (2 | 8)).all() and v[192:].tolist() == [13, 13, 15, 13]
    assert line_prompt_classes(64, 64, OVERLAP, 4, has_prompt=[False, False]) is None
    with pytest.raises(ValueError, match="entries for"):
        line_prompt_classes(64, 64, OVERLAP, 4, has_prompt=[True])


def test_batch_two_with_per_image_masks_under_true_cfg():
    from reptext_amd.pipeline import line_prompt_classes

    per_image = [torch.stack([OVERLAP[0], OVERLAP[1]]).reshape(2, 4, 1), OVERLAP[1].reshape(1, 4, 1)]
    row_vis, key_class = line_prompt_classes(64, 64, per_image, 4, batch=2, cfg=True)
    v, kc = words(row_vis), key_class.numpy()
    assert v.shape == kc.shape == (4, 196)
    # image 0: memberships [{1}, {}, {1,2}, {}]; image 1: line 1's box is line 2's, [{}, {}, {1,2}, {}]. One numbering for the batch.
    assert kc[2, 192:].tolist() == [4, 3, 5, 3] and kc[3, 192:].tolist() == [3, 3, 5, 3]
    assert (kc[:2] == kc[2:]).all()                                      # the negative half's keys carry the positive half's classes
    assert v[2, 192:].tolist() == [59, 57, 63, 57] and v[3, 192:].tolist() == [57, 57, 63, 57]
    assert (v[:2, 192:] == 57).all()                                     # the negative half's image rows: the base prompt and all image classes
    assert (v[:, :64] == 57).all() and (v[:, 64:128] == 50).all() and (v[:, 128:192] == 36).all()
    assert sees_a_key(row_vis, key_class)
    single = line_prompt_classes(64, 64, OVERLAP, 4, cfg=True)
    assert (words(single[0])[1] == words(line_prompt_classes(64, 64, OVERLAP, 4)[0])[0]).all() and sees_a_key(*single)
    with pytest.raises(ValueError, match="batch of 3"):
        line_prompt_classes(64, 64, per_image, 4, batch=3)


def test_the_33rd_class_is_refused():
    from reptext_amd.pipeline import line_prompt_classes

    one_hot = lambda n, N, *more: torch.tensor([1.0 if i in (n,) + more else 0.0 for i in range(N)])
    row_vis, key_class = line_prompt_classes(64, 64, [one_hot(r, 16) for r in range(15)], 16)       # 1 + 15 + 1 + 15 = 32
    assert int(key_class.max()) == 31 and sees_a_key(row_vis, key_class)
    assert int(words(row_vis)[0, 0]) == (1 | (0xFFFF << 16)) and int(words(row_vis)[0, -1]) == (1 | (0xFFFF << 16))
    assert int(words(row_vis)[0, 64 + 15 * 64 + 14]) == (1 | 1 << 15 | 1 << 16 | 1 << 31)
    with pytest.raises(ValueError, match="34 key classes"):
        line_prompt_classes(64, 64, [one_hot(r, 16) for r in range(16)], 16)
    # 15 boxes and ONE overlap (token 16 lies in boxes 1 and 2): the 33rd class
    masks = [one_hot(0, 17, 16), one_hot(1, 17, 16)] + [one_hot(r, 17) for r in range(2, 15)]
    with pytest.raises(ValueError, match="33 key classes"):
        line_prompt_classes(64, 64, masks, 17)


def test_the_records():
    from reptext_amd import ops, pipeline
    from reptext_amd.pipeline import (CallExtensions, IsolatedLinePrompts, IsolationCallExtensions, LineCallExtensions, LinePrompts, LoopExtras,
                                      RegionalIPCallExtensions)

    names = [f.name for f in dataclasses.fields(IsolationCallExtensions)]
    assert tuple(names[-1:]) == pipeline.ISOLATION_ARGUMENTS == ("control_prompt_isolation",) and IsolationCallExtensions().control_prompt_isolation is False
    assert names[:-1] == [f.name for f in dataclasses.fields(RegionalIPCallExtensions)] and issubclass(IsolationCallExtensions, RegionalIPCallExtensions)
    assert tuple(f.name for f in dataclasses.fields(LineCallExtensions))[-3:] == pipeline.LINE_PROMPT_ARGUMENTS
    assert tuple(f.name for f in dataclasses.fields(RegionalIPCallExtensions))[-4:] == pipeline.REGIONAL_IP_ARGUMENTS
    assert len(dataclasses.fields(RegionalIPCallExtensions)) == 13 + 3 + 4
    # only a call that names the keyword carries the new record
    pipe = _pipe()
    seen = []
    pipe.check_inputs = lambda *a, **k: seen.append(pipe._call_extensions)
    for kw in (dict(control_prompt=["x"], control_prompt_isolation=True), dict(control_prompt=["x"]), dict(ip_adapter_mask="m"), {}):
        with pytest.raises(Exception):
            pipe(**dict(_kw(), prompt_embeds=None), **kw)
    assert [type(s) for s in seen] == [IsolationCallExtensions, LineCallExtensions, RegionalIPCallExtensions, CallExtensions]
    assert seen[0] == IsolationCallExtensions(control_prompt=["x"], control_prompt_isolation=True) and pipe._call_extensions is None
    # the class table travels in the line_prompts slot
    emb, vis, kc = torch.zeros(2, 128, 48), torch.zeros(2, 208, dtype=torch.int32), torch.zeros(2, 208, dtype=torch.uint8)
    sig = lambda t: ("sig", tuple(t.shape), str(t.dtype))
    plain, iso = LinePrompts(emb, (64, 192, 208), vis), IsolatedLinePrompts(emb, (64, 192, 208), vis, kc)
    assert [f.name for f in dataclasses.fields(iso)] == [f.name for f in dataclasses.fields(plain)] + ["key_class"]
    assert LinePrompts.STATIC == {"line_embeds": "embeds", "line_row_vis": "row_vis"}
    assert IsolatedLinePrompts.STATIC == {"line_embeds": "embeds", "line_row_vis": "row_vis", "line_key_class": "key_class"}
    assert iso.signature(sig) == plain.signature(sig) + (("line_isolation", sig(kc)),)
    assert LoopExtras(line_prompts=iso).signature(sig, None, None) == iso.signature(sig) != LoopExtras(line_prompts=plain).signature(sig, None, None)
    assert list(LoopExtras(line_prompts=iso).tensors()) == ["line_embeds", "line_row_vis", "line_key_class"]
    static = {k: t.clone() for k, t in iso.tensors().items()}
    bound = LoopExtras(line_prompts=iso).rebound(static).line_prompts
    assert type(bound) is IsolatedLinePrompts and bound.key_class is static["line_key_class"] and bound.row_vis is static["line_row_vis"]
    g, half = iso.groups(), iso.groups(slice(1, 2))
    assert type(g) is ops.KeyClasses and g.row_vis is vis and g.key_class is kc and type(plain.groups()) is ops.KeyGroups
    assert half.row_vis.shape == half.key_class.shape == (1, 208) and half.key_class.data_ptr() == kc[1:].data_ptr()


def test_key_classes_checks_once_at_construction():
    from reptext_amd import ops

    vis, kc = torch.zeros(1, 8, dtype=torch.int32), torch.zeros(1, 8, dtype=torch.uint8)
    with pytest.raises(TypeError, match="key_class must be a uint8"):
        ops.KeyClasses(vis, kc.to(torch.int32))
    with pytest.raises(TypeError, match="row_vis must be an int32"):
        ops.KeyClasses(vis.float(), kc)
    with pytest.raises(ValueError, match="unit inner stride"):
        ops.KeyClasses(vis, torch.zeros(1, 16, dtype=torch.uint8)[:, ::2])
    with pytest.raises(ValueError, match="unit inner stride"):
        ops.KeyClasses(vis, torch.zeros(1, 9, dtype=torch.uint8))
    bad = kc.clone()
    bad[0, 5] = 32
    with pytest.raises(ValueError, match="below 32, got 32"):
        ops.KeyClasses(vis, bad)
    with pytest.raises(ValueError, match=r"need \[2 or 1, 9\]"):
        ops.KeyClasses(vis, kc).check(2, 9)
    with pytest.raises(ValueError, match=r"need \[3 or 1, 8\]"):
        ops.KeyClasses(vis.expand(2, 8).contiguous(), kc).check(3, 8)


def test_the_refusals(no_native_call):
    from reptext_amd.pipeline import IsolationCallExtensions, line_isolation_argument

    assert line_isolation_argument(IsolationCallExtensions(), None) is False and line_isolation_argument(object(), ["a"]) is False
    assert line_isolation_argument(IsolationCallExtensions(control_prompt_isolation=True), ["a", None]) is True
    with pytest.raises(ValueError, match="needs a per-line prompt"):
        line_isolation_argument(IsolationCallExtensions(control_prompt_isolation=True), None)
    with pytest.raises(ValueError, match="must be a bool"):
        line_isolation_argument(IsolationCallExtensions(control_prompt_isolation=1), ["a"])
    pipe = _pipe()
    hint = [torch.zeros(1, 16, 128)]
    with pytest.raises(ValueError, match="needs a per-line prompt"):
        pipe(**_kw(), control_image=hint, control_mask=[torch.zeros(1, 16, 1)], control_prompt_isolation=True)
    with pytest.raises(ValueError, match="needs a per-line prompt"):
        pipe(**_kw(), control_image=hint, control_mask=[torch.zeros(1, 16, 1)], control_prompt=[None], control_prompt_isolation=True)
    with pytest.raises(ValueError, match="control_mask"):                    # what line_prompt_arguments refuses stays refused
        pipe(**_kw(), control_image=hint, control_prompt=["white chalk"], control_prompt_isolation=True)
    pipe.transformer._fp8_attention = True
    with pytest.raises(ValueError, match="enable_fp8_attention"):
        pipe(**_kw(), control_image=hint, control_prompt_embeds=[torch.zeros(1, 128, 64)], control_mask=[torch.zeros(1, 16, 1)],
             control_prompt_isolation=True)
    assert_no_call_state(pipe)
    with pytest.raises(ValueError, match="inpaint pipeline does not support per-line prompts"):
        _pipe(inpaint=True)(**_kw(), control_prompt_isolation=True)


def test_the_launch_stream_differs_by_the_attention_entry_alone():
    """One double and one single block with key groups, then with key classes over the same rows: the same native calls in the same
    order on the same buffers; the two attention launches are rt_attention_fwd_keyed instead of rt_attention_fwd_grouped, with the same
    q, k, v, o, strides, shape, scale, row table and workspace arguments."""
    import block_launch_recorder as blr
    from reptext_amd import mmdit, ops

    class Rec(blr.Recorder):
        def pointer(self, ptr):
            return "host" if isinstance(ptr, C.c_void_p) else super().pointer(ptr)      # the group ends: a host array

    H = 2
    d, S = H * 128, blr.T + blr.N

    def record(keyed):
        rec = Rec()
        with blr.recording(rec):
            dbl, sgl = blr.blocks(H)
            rec.blocks = {"double": dbl, "single": sgl}
            pd, ps = mmdit.plan_double(dbl), mmdit.plan_single(sgl)
            ws = mmdit.Workspace(blr.B, blr.T, blr.N, d, torch.device("cpu"), True)
            temb, cos, sin = rec.new(blr.B, d, dtype=blr.F32), rec.new(S, 128, dtype=blr.F32), rec.new(S, 128, dtype=blr.F32)
            vis = rec.track(torch.full((blr.B, S), 7, dtype=torch.int32))
            cls = rec.track(torch.zeros(blr.B, S, dtype=torch.uint8))
            assert [rec.pointer(vis.data_ptr()), rec.pointer(cls.data_ptr())] == ["b0+0", "b1+0"]       # named alike in both streams
            groups = ops.KeyClasses(vis, cls) if keyed else ops.KeyGroups((blr.T, S), vis)
            mmdit.run_double(pd, ws, temb, cos, sin, H, groups=groups)
            mmdit.run_single(ps, ws, temb, cos, sin, H, groups=groups)
        return rec.lines

    grouped, keyed = record(False), record(True)
    name = lambda line: line.split("(", 1)[0]
    args = lambda line: line.split("(", 1)[1][:-1].split(", ")
    assert [name(x) for x in keyed] == [name(x).replace("rt_attention_fwd_grouped", "rt_attention_fwd_keyed") for x in grouped]
    assert sum(name(x) == "rt_attention_fwd_grouped" for x in grouped) == 2 == sum(name(x) == "rt_attention_fwd_keyed" for x in keyed)
    assert not any("attention_fwd_grouped" in x for x in keyed)
    for g, k in zip(grouped, keyed):
        if name(g) != "rt_attention_fwd_grouped":
            assert g == k
            continue
        ga, ka = args(g), args(k)
        # (q, k, v, o, ld, stride_b, ldo, stride_ob, B, S, H, scale | ends, n, vis, stride | vis, stride, classes, stride | ws, bytes, stream)
        assert ga[:12] == ka[:12] and ga[-3:] == ka[-3:] and ga[12:16] == ["host", "2", "b0+0", repr(S)]
        assert ka[12:16] == ["b0+0", repr(S), "b1+0", repr(S)]
