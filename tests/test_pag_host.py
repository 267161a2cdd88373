"""Host side of perturbed-attention guidance (``pag_scale`` / ``pag_applied_layers``): the known answers of ``pipeline.pag_layers`` and
``pipeline.perturbed_attention_tables`` written out by hand; every refusal of a call, by name and before any native call; the record
that carries the keywords and the one that carries the tables; the graph key; that a call without the keywords builds what it built
before; and ``ops.attention``'s argument refusals for ``self_key``. No kernel runs."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_true_cfg_host import _kw, _pipe, assert_no_call_state, no_native_call  # noqa: E402,F401


def test_known_answers_of_the_layer_names():
    from reptext_amd.pipeline import pag_layers

    assert pag_layers(["transformer_blocks.8"], 19, 38) == (frozenset({8}), frozenset())
    assert pag_layers(("single_transformer_blocks.0", "transformer_blocks.18", "transformer_blocks.0", "single_transformer_blocks.37"), 19, 38) == \
        (frozenset({0, 18}), frozenset({0, 37}))
    assert pag_layers(["single_transformer_blocks.3"], 0, 4) == (frozenset(), frozenset({3}))
    for bad in (["transformer_blocks.19"], ["single_transformer_blocks.38"], ["transformer_blocks.0"] * 2,
                ["transformer_blocks.1", "single_transformer_blocks.2", "transformer_blocks.1"], [], (), "transformer_blocks.1", None, 8, [8],
                ["blocks.1"], ["transformer_blocks"], ["transformer_blocks."], ["transformer_blocks.-1"], ["transformer_blocks.1.attn"],
                ["transformer_blocks.01"], ["transformer_blocks.x"], ["transformer.transformer_blocks.1"], ["Transformer_blocks.1"],
                ["transformer_blocks.1 "], ["transformer_blocks.٣"]):
        with pytest.raises(ValueError, match="pag_applied_layers"):
            pag_layers(bad, 19, 38)
    with pytest.raises(ValueError, match="out of range, the model has 19 transformer_blocks"):
        pag_layers(["transformer_blocks.19"], 19, 38)
    with pytest.raises(ValueError, match="named twice"):
        pag_layers(["single_transformer_blocks.5", "single_transformer_blocks.5"], 19, 38)
    with pytest.raises(ValueError, match="empty"):
        pag_layers([], 19, 38)


@pytest.mark.parametrize("B", [1, 2])
def test_known_answers_of_the_tables(B):
    from reptext_amd.pipeline import perturbed_attention_tables

    T, N = 64, 128
    row_vis, key_class = perturbed_attention_tables(T, N, B)
    assert row_vis.dtype == torch.int32 and tuple(row_vis.shape) == (2 * B, T + N) and row_vis.is_contiguous()
    assert key_class.dtype == torch.uint8 and tuple(key_class.shape) == (1, T + N) and key_class.is_contiguous()
    assert key_class[0].tolist() == [0] * 64 + [1] * 128                                # class 0: the text keys, class 1: the image keys
    for b in range(B):                                                                  # the perturbed half comes first
        assert row_vis[b].tolist() == [3] * 64 + [1] * 128                              # a text row sees all, an image row the text keys
        assert row_vis[B + b].tolist() == [3] * 192                                     # the positive half sees everything
    # what the launch with the self rule then shows row i: bit class[j] of its word, or j == i
    see = ((row_vis.numpy().view(np.uint32)[:, :, None] >> key_class.numpy()[:, None, :].astype(np.uint32)) & 1).astype(bool) | np.eye(T + N, dtype=bool)
    assert see[0, :T].all() and see[B:].all()
    assert (see[0, T:, :T]).all() and (see[0, T:, T:] == np.eye(N, dtype=bool)).all()   # text, and its own key alone among the image keys
    with pytest.raises(ValueError):
        perturbed_attention_tables(0, 0, 1)
    with pytest.raises(ValueError):
        perturbed_attention_tables(64, 128, 0)
    assert perturbed_attention_tables(64, 0, 1)[0].tolist() == [[3] * 64] * 2


def test_the_argument_rule():
    from types import SimpleNamespace

    from reptext_amd.pipeline import PerturbedCallExtensions as Ext, pag_arguments

    tr = SimpleNamespace(transformer_blocks=[0] * 19, single_transformer_blocks=[0] * 38)
    assert pag_arguments(Ext(), tr, False) is None and pag_arguments(object(), tr, True) is None
    assert pag_arguments(Ext(pag_scale=0.0, pag_applied_layers=["transformer_blocks.8"]), tr, True) is None          # off: the plain call
    assert pag_arguments(Ext(pag_scale=3.0, pag_applied_layers=["transformer_blocks.8"]), tr, False) == (4.0, frozenset({8}), frozenset())
    # 1 + pag_scale is formed in double, not in fp32
    s = pag_arguments(Ext(pag_scale=0.1, pag_applied_layers=["single_transformer_blocks.1"]), tr, False)
    assert s == (1.0 + 0.1, frozenset(), frozenset({1})) and s[0] != float(np.float32(1.0) + np.float32(0.1))
    assert pag_arguments(Ext(pag_scale=2, pag_applied_layers=["transformer_blocks.0"]), tr, False)[0] == 3.0
    for bad in (-1.0, -0.0001, float("inf"), float("-inf"), float("nan"), "3.0", None, True, [3.0], torch.tensor(3.0)):
        with pytest.raises(ValueError, match="pag_scale must be a finite number >= 0"):
            pag_arguments(Ext(pag_scale=bad, pag_applied_layers=["transformer_blocks.8"]), tr, False)
    with pytest.raises(ValueError, match="needs pag_applied_layers"):
        pag_arguments(Ext(pag_scale=3.0), tr, False)
    with pytest.raises(ValueError, match="out of range"):                              # named layers are checked even when PAG is off
        pag_arguments(Ext(pag_applied_layers=["transformer_blocks.19"]), tr, False)


def test_the_refusals_of_a_call(no_native_call):
    pipe = _pipe()                          # 2 double blocks, 1 single block
    layers = ["transformer_blocks.1"]
    hint, mask = [torch.zeros(1, 16, 128)], [torch.zeros(1, 16, 1)]
    emb = [torch.zeros(1, 128, 64)]
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="pag_scale must be a finite number >= 0"):
            pipe(**_kw(), pag_scale=bad, pag_applied_layers=layers)
    with pytest.raises(ValueError, match="needs pag_applied_layers"):
        pipe(**_kw(), pag_scale=3.0)
    for bad, msg in (([], "empty"), (["transformer_blocks.2"], "out of range"), (["single_transformer_blocks.1"], "out of range"),
                     (layers * 2, "named twice"), (["attn.1"], "neither"), ("transformer_blocks.1", "must be a list")):
        with pytest.raises(ValueError, match=msg):
            pipe(**_kw(), pag_scale=3.0, pag_applied_layers=bad)
    with pytest.raises(ValueError, match="negative prompt"):
        pipe(**_kw(), pag_scale=3.0, pag_applied_layers=layers, true_cfg_scale=2.0, negative_prompt_embeds=torch.zeros(1, 8, 64),
             negative_pooled_prompt_embeds=torch.zeros(1, 32))
    line_kw = dict(control_image=hint, control_mask=mask)
    for kw, name in ((dict(control_prompt_embeds=emb), "control_prompt_embeds"), (dict(control_prompt=["x"]), "control_prompt"),
                     (dict(control_prompt_embeds=emb, control_prompt_isolation=True), "control_prompt_isolation"),
                     (dict(control_prompt_embeds=emb, control_prompt_scale=2.0), "control_prompt_scale"),
                     (dict(control_ip_adapter_image_embeds=[torch.zeros(1, 32)]), "control_ip_adapter_image_embeds")):
        with pytest.raises(ValueError, match=f"pag_scale cannot be combined with per-line prompts .*{name}"):
            pipe(**_kw(), **line_kw, **kw, pag_scale=3.0, pag_applied_layers=layers)
    pipe.transformer._fp8_attention = True
    with pytest.raises(ValueError, match="enable_fp8_attention"):
        pipe(**_kw(), pag_scale=3.0, pag_applied_layers=layers)
    pipe.transformer._fp8_attention = False
    assert_no_call_state(pipe)
    for kw in (dict(pag_scale=3.0), dict(pag_applied_layers=layers), dict(pag_scale=3.0, pag_applied_layers=layers)):
        with pytest.raises(ValueError, match=r"inpaint pipeline does not support perturbed-attention guidance \(pag_scale / pag_applied_layers\)"):
            _pipe(inpaint=True)(**_kw(), **kw)
    with pytest.raises(TypeError):                                           # still no such keyword as a misspelt one
        pipe(**_kw(), pag_scales=3.0)


def test_the_records():
    from reptext_amd import pipeline
    from reptext_amd.pipeline import (CallExtensions, LineScale, LineScaleCallExtensions, LoopExtras, Perturbed, PerturbedCallExtensions,
                                      perturbed_attention_tables)

    names = [f.name for f in dataclasses.fields(PerturbedCallExtensions)]
    assert tuple(names[-2:]) == pipeline.PAG_ARGUMENTS == ("pag_scale", "pag_applied_layers")
    assert PerturbedCallExtensions().pag_scale == 0.0 and PerturbedCallExtensions().pag_applied_layers is None
    assert names[:-2] == [f.name for f in dataclasses.fields(LineScaleCallExtensions)] and issubclass(PerturbedCallExtensions, LineScaleCallExtensions)
    assert len(dataclasses.fields(CallExtensions)) == 13 and len(dataclasses.fields(LineScaleCallExtensions)) == 22      # what they were
    # only a call that names a keyword carries the new record; every other call the record it carried
    pipe = _pipe()
    seen = []
    pipe.check_inputs = lambda *a, **k: seen.append(pipe._call_extensions)
    for kw in (dict(pag_scale=3.0), dict(pag_applied_layers=["transformer_blocks.0"]), dict(control_prompt=["x"], control_prompt_scale=[2.0]), {}):
        with pytest.raises(Exception):
            pipe(**dict(_kw(), prompt_embeds=None), **kw)
    assert [type(s) for s in seen] == [PerturbedCallExtensions, PerturbedCallExtensions, LineScaleCallExtensions, CallExtensions]
    assert seen[0] == PerturbedCallExtensions(pag_scale=3.0) and seen[3] == CallExtensions() and pipe._call_extensions is None
    # the tables travel in a slot of their own as two static inputs; the key part comes last
    row_vis, key_class = perturbed_attention_tables(64, 128, 1)
    sig = lambda t: ("sig", tuple(t.shape), str(t.dtype))
    rec = Perturbed(row_vis, key_class, frozenset({8, 2}), frozenset({11, 3}))
    assert [f.name for f in dataclasses.fields(Perturbed)] == ["row_vis", "key_class", "double_ids", "single_ids"]
    assert Perturbed.STATIC == {"pag_row_vis": "row_vis", "pag_key_class": "key_class"}
    layers = ("transformer_blocks.2", "transformer_blocks.8", "single_transformer_blocks.3", "single_transformer_blocks.11")
    assert rec.signature(sig) == (("pag", layers, sig(row_vis), sig(key_class)),)
    assert LoopExtras().perturbed is None and LoopExtras().signature(sig, None, None) == () and LoopExtras().tensors() == {}
    without, with_ = LoopExtras(cfg_scale=4.0), LoopExtras(cfg_scale=4.0, perturbed=rec)
    assert without.signature(sig, None, None) == (("cfg", 4.0),)
    assert with_.signature(sig, None, None) == (("cfg", 4.0),) + rec.signature(sig)
    table = torch.zeros(1, 32)
    assert LoopExtras(perturbed=rec, line_scale=LineScale(table)).signature(sig, None, None)[-1] == rec.signature(sig)[0]      # appended, last
    assert list(with_.tensors()) == ["pag_row_vis", "pag_key_class"] and with_.tensors()["pag_row_vis"] is row_vis
    static = {k: t.clone() for k, t in with_.tensors().items()}
    bound = with_.rebound(static)
    assert type(bound.perturbed) is Perturbed and bound.perturbed.row_vis is static["pag_row_vis"] and bound.perturbed.key_class is static["pag_key_class"]
    assert bound.perturbed.double_ids == rec.double_ids and bound.signature(sig, None, None) == with_.signature(sig, None, None)
    assert without.rebound({}).perturbed is None
    groups = rec.groups()
    assert groups.row_vis is row_vis and groups.key_class is key_class
    # another layer set is another graph; another pag_scale is another ("cfg", s)
    other = Perturbed(row_vis, key_class, frozenset({8}), frozenset({11, 3}))
    assert other.signature(sig) != rec.signature(sig)


def _record(perturbed, H=2):
    """The launch stream of one double and one single block: as today, or under key classes with the self rule."""
    import block_launch_recorder as blr
    from reptext_amd import mmdit, ops

    d, S = H * 128, blr.T + blr.N
    rec = blr.Recorder()
    with blr.recording(rec):
        dbl, sgl = blr.blocks(H)
        rec.blocks = {"double": dbl, "single": sgl}
        pd, ps = mmdit.plan_double(dbl), mmdit.plan_single(sgl)
        ws = mmdit.Workspace(blr.B, blr.T, blr.N, d, torch.device("cpu"), True)
        temb, cos, sin = rec.new(blr.B, d, dtype=blr.F32), rec.new(S, 128, dtype=blr.F32), rec.new(S, 128, dtype=blr.F32)
        vis = rec.track(torch.full((blr.B, S), 3, dtype=torch.int32))
        cls = rec.track(torch.zeros(1, S, dtype=torch.uint8))
        kw = {} if perturbed is None else dict(groups=ops.KeyClasses(vis, cls), **({"self_key": True} if perturbed else {}))
        mmdit.run_double(pd, ws, temb, cos, sin, H, **kw)
        mmdit.run_single(ps, ws, temb, cos, sin, H, **kw)
    return rec.lines


def test_the_launch_stream_differs_by_the_attention_entry_alone():
    """The same native calls in the same order; the two attention launches are rt_attention_fwd_keyed_self with the keyed entry's
    arguments. Against the plain blocks the attention launches alone differ."""
    plain, keyed, selfk = _record(None), _record(False), _record(True)
    name = lambda line: line.split("(", 1)[0]
    assert [name(x) for x in selfk] == [name(x) + "_self" if name(x) == "rt_attention_fwd_keyed" else name(x) for x in keyed]
    assert sum(name(x) == "rt_attention_fwd_keyed_self" for x in selfk) == 2 and not any("_self" in x for x in keyed + plain)
    for k, s in zip(keyed, selfk):
        assert s == (k.replace("rt_attention_fwd_keyed(", "rt_attention_fwd_keyed_self(", 1) if name(k) == "rt_attention_fwd_keyed" else k)
    dense = lambda n: "rt_attention_fwd_rows" if n == "rt_attention_fwd_keyed_self" else n
    assert [name(x) for x in plain] == [dense(name(x)) for x in selfk]


def test_run_blocks_refuse_the_self_rule_without_groups():
    import block_launch_recorder as blr
    from reptext_amd import mmdit

    rec = blr.Recorder()
    with blr.recording(rec):
        dbl, sgl = blr.blocks(2)
        rec.blocks = {"double": dbl, "single": sgl}
        pd, ps = mmdit.plan_double(dbl), mmdit.plan_single(sgl)
        ws = mmdit.Workspace(blr.B, blr.T, blr.N, 256, torch.device("cpu"), True)
        temb, cos, sin = rec.new(blr.B, 256, dtype=blr.F32), rec.new(192, 128, dtype=blr.F32), rec.new(192, 128, dtype=blr.F32)
        with pytest.raises(ValueError, match="self_key needs key groups"):
            mmdit.run_double(pd, ws, temb, cos, sin, 2, self_key=True)
        with pytest.raises(ValueError, match="self_key needs key groups"):
            mmdit.run_single(ps, ws, temb, cos, sin, 2, self_key=True)


def test_the_op_refuses_before_any_native_call(no_native_call):
    """``ops.attention``'s refusals for ``self_key``: it belongs to the per-key launch alone."""
    from reptext_amd import ops

    B, S, H = 2, 128, 1
    buf = torch.zeros(B, S, 3 * 128, dtype=torch.bfloat16)
    q, k, v = buf[..., :128], buf[..., 128:256], buf[..., 256:]
    groups = ops.KeyGroups((64, 128), torch.zeros(1, S, dtype=torch.int32))
    keyed = ops.KeyClasses(torch.zeros(1, S, dtype=torch.int32), torch.zeros(1, S, dtype=torch.uint8))
    for kw in (dict(), dict(groups=groups), dict(groups=keyed, rows=(0, 64)), dict(groups=keyed, key_bias=torch.zeros(1, 32)),
               dict(rows=(0, 64)), dict(groups=groups, key_bias=torch.zeros(1, 32))):
        with pytest.raises(ValueError, match="self_key=True needs groups= as a KeyClasses"):
            ops.attention(q, k, v, q, H, self_key=True, **kw)
    assert [f.name for f in dataclasses.fields(ops.KeyClasses)] == ["row_vis", "key_class"]             # the record gains nothing


def test_the_binding_comes_from_the_header():
    from reptext_amd import native

    assert native.SIGNATURES["rt_attention_fwd_keyed_self"] == native.SIGNATURES["rt_attention_fwd_keyed"]      # the keyed entry's arguments
    assert native.RESTYPES["rt_attention_fwd_keyed_self"] == native.RESTYPES["rt_attention_fwd_keyed"]
    assert native.ABI_VERSION == 15
