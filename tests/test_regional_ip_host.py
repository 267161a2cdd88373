"""Host side of regional image prompts: the known answers of ``ip_adapter.regional_ip_weights`` (the one rule for the row weights), the
refusals of the new keywords by name and before any native call, the record that carries them, and the native call ``row_weights``
makes. No kernel runs."""
import dataclasses
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ip_adapter_reference as ipr  # noqa: E402
from test_true_cfg_host import CFG, E, _kw, _pipe, assert_no_call_state, no_native_call  # noqa: E402,F401


def test_known_answers_of_the_weight_rule():
    from reptext_amd.ip_adapter import regional_ip_weights as rule

    N = 4
    # the call's own prompt without a mask: no table, the unweighted launch
    assert rule(None, N=N) == (None, None)
    with pytest.raises(ValueError, match="regional mask"):
        rule(None, N=N, line=True)
    # a full mask: all ones, text value 1 (the unmasked call); an empty one: zeros
    img, txt = rule(torch.ones(1, N, 1), N=N)
    assert img.dtype == txt.dtype == torch.float32 and img.shape == (1, N) and txt.shape == (1,)
    assert img.tolist() == [[1.0] * N] and txt.tolist() == [1.0]
    img, txt = rule(torch.zeros(N), 0.7, N=N, line=True)
    assert img.tolist() == [[0.0] * N] and txt.tolist() == [0.0]
    # a fractional edge keeps its resized value times the scale; the text rows leak in proportion to the area
    m = torch.tensor([1.0, 0.5, 0.25, 0.0])
    img, txt = rule(m.reshape(1, N, 1), 2.0, N=N, line=True)
    assert img.tolist() == [[2.0, 1.0, 0.5, 0.0]] and txt.tolist() == [2.0 * 1.75 / 4]
    img, txt = rule(m.to(torch.bfloat16), -1.5, N=N, line=True)             # the mask in the prompt's dtype; negative scales fold in
    assert img.tolist() == [[-1.5, -0.75, -0.375, 0.0]] and txt.tolist() == [-1.5 * 1.75 / 4]
    # true CFG: [negative, positive]. A line's term weighs nothing in the negative half; the call's own prompt carries its mask in both
    img, txt = rule(m, 0.5, N=N, cfg=True, line=True)
    assert img.tolist() == [[0.0] * N, [0.5, 0.25, 0.125, 0.0]] and txt.tolist() == [0.0, 0.5 * 1.75 / 4]
    img, txt = rule(m, N=N, cfg=True)
    assert img.tolist() == [m.tolist(), m.tolist()] and txt.tolist() == [1.75 / 4] * 2
    # per-sample masks [B, N, 1], alone and under true CFG (negative half first, B entries each)
    per = torch.stack([m, m.flip(0)]).reshape(2, N, 1)
    img, txt = rule(per, N=N, batch=2, line=True)
    assert img.tolist() == [m.tolist(), m.flip(0).tolist()] and txt.tolist() == [1.75 / 4] * 2
    img, txt = rule(per, N=N, batch=2, cfg=True, line=True)
    assert img.shape == (4, N) and not img[:2].any() and img[2:].tolist() == [m.tolist(), m.flip(0).tolist()] and txt.tolist() == [0, 0, 1.75 / 4, 1.75 / 4]
    img, _ = rule(m, N=N, batch=2, cfg=True)                                 # a shared mask serves every entry of both halves
    assert img.shape == (4, N) and (img == m).all()
    with pytest.raises(ValueError, match="batch of 2"):
        rule(torch.zeros(3, N, 1), N=N, batch=2)
    # scale 0.5 with m equals scale 1 with m / 2
    a, b = rule(m, 0.5, N=N, line=True), rule(m / 2, 1.0, N=N, line=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


class _Adapter:
    E = E
    active = True


def test_the_argument_errors(no_native_call):
    from reptext_amd.pipeline import RegionalIPCallExtensions as R, regional_ip_arguments as check

    masks, e = ["m0", "m1"], torch.zeros(1, E)
    assert check(R(), 2, masks, _Adapter, False, False) is None
    assert check(R(control_ip_adapter_scale=0.3), 2, masks, None, False, False) is None          # a scale alone names no image prompt
    got = check(R(control_ip_adapter_image_embeds=[e, None], control_ip_adapter_scale=[0.5, 2]), 2, masks, _Adapter, False, False)
    assert got[0][0] is e and got[0][1] is None and got[1] == [0.5, 2.0] and got[2] is None
    got = check(R(control_ip_adapter_image_embeds=[torch.zeros(2, 1, E), None]), 2, masks, _Adapter, False, False)
    assert got[0][0].shape == (2, E) and got[1] == [1.0, 1.0]
    assert check(R(ip_adapter_mask="m"), 2, None, _Adapter, True, False) == ([None, None], [1.0, 1.0], "m")
    assert check(R(control_ip_adapter_image_embeds=[None, None]), 2, None, _Adapter, False, False)[0] == [None, None]
    pixels = torch.zeros(3, 8, 8)
    assert check(R(control_ip_adapter_image=[pixels, None]), 2, masks, _Adapter, False, True)[0][0] is pixels
    for ext, n_lines, m, adapter, positive, match in (
            (R(control_ip_adapter_image_embeds=[e]), 2, masks, _Adapter, False, "one entry per text line"),
            (R(control_ip_adapter_image_embeds=e), 1, masks[:1], _Adapter, False, "one entry per text line"),
            (R(control_ip_adapter_image=[pixels] * 3), 2, masks, _Adapter, False, "one entry per text line"),
            (R(control_ip_adapter_image_embeds=[e, "photo.png"]), 2, masks, _Adapter, False, r"\[1,E\] tensor or None"),
            (R(control_ip_adapter_image_embeds=[torch.zeros(1, 2, E), None]), 2, masks, _Adapter, False, r"\[1,E\] tensor or None"),
            (R(control_ip_adapter_image=[7, None]), 2, masks, _Adapter, False, "an entry is an image"),
            (R(control_ip_adapter_image_embeds=[torch.zeros(1, E + 8), None]), 2, masks, _Adapter, False, "embedding width"),
            (R(control_ip_adapter_image_embeds=[e, None]), 2, None, _Adapter, False, "needs control_mask"),
            (R(control_ip_adapter_image_embeds=[e, None]), 2, masks, None, False, "no IP-Adapter is loaded"),
            (R(ip_adapter_mask="m"), 2, masks, None, True, "no IP-Adapter is loaded"),
            (R(ip_adapter_mask="m"), 2, masks, _Adapter, False, "without an image prompt"),
            (R(control_ip_adapter_image=[pixels, None], control_ip_adapter_image_embeds=[e, None]), 2, masks, _Adapter, False, "not both"),
            (R(control_ip_adapter_image_embeds=[e, None], control_ip_adapter_scale=[1.0]), 2, masks, _Adapter, False, "one float per text line"),
            (R(control_ip_adapter_image_embeds=[e, None], control_ip_adapter_scale="1"), 2, masks, _Adapter, False, "one float per text line")):
        with pytest.raises(ValueError, match=match):
            check(ext, n_lines, m, adapter, positive, False)
    with pytest.raises(NotImplementedError, match="needs an image encoder"):
        check(R(control_ip_adapter_image=[pixels, None]), 2, masks, _Adapter, False, False)


def _with_adapter(pipe):
    p = ipr.init_ip_params(CFG, 4, E, seed=3)
    pipe.transformer.load_ip_adapter({k: v.to(torch.bfloat16) for k, v in p.items()})
    return pipe


def test_the_pipelines_refuse_before_any_kernel(no_native_call):
    hint, mask, e = [torch.zeros(1, 16, 128)], [torch.zeros(1, 16, 1)], torch.zeros(1, E)
    pipe = _pipe()
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        pipe(**_kw(), control_image=hint, control_mask=mask, control_ip_adapter_image_embeds=[e])
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        pipe(**_kw(), ip_adapter_mask=mask[0])
    assert_no_call_state(pipe)
    pipe = _with_adapter(_pipe())
    with pytest.raises(ValueError, match="needs control_mask"):
        pipe(**_kw(), control_image=hint, control_ip_adapter_image_embeds=[e])
    with pytest.raises(ValueError, match="one entry per text line"):
        pipe(**_kw(), control_image=hint, control_mask=mask, control_ip_adapter_image_embeds=[e, e])
    with pytest.raises(ValueError, match="embedding width"):
        pipe(**_kw(), control_image=hint, control_mask=mask, control_ip_adapter_image_embeds=[torch.zeros(1, E + 8)])
    with pytest.raises(ValueError, match="without an image prompt"):
        pipe(**_kw(), ip_adapter_mask=mask[0])
    with pytest.raises(ValueError, match="not both"):
        pipe(**_kw(), control_image=hint, control_mask=mask, control_ip_adapter_image_embeds=[e], control_ip_adapter_image=[torch.zeros(3, 8, 8)])
    with pytest.raises(NotImplementedError, match="needs an image encoder"):
        pipe(**_kw(), control_image=hint, control_mask=mask, control_ip_adapter_image=[torch.zeros(3, 8, 8)])
    assert_no_call_state(pipe)
    with pytest.raises(ValueError, match="inpaint pipeline does not support IP-Adapter image prompts"):
        _pipe(inpaint=True)(**_kw(), control_ip_adapter_image_embeds=[e])
    with pytest.raises(ValueError, match="inpaint pipeline does not support IP-Adapter image prompts"):
        _pipe(inpaint=True)(**_kw(), ip_adapter_mask=mask[0])


def test_the_record_carries_the_new_fields():
    from reptext_amd import pipeline
    from reptext_amd.pipeline import CallExtensions, LineCallExtensions, LoopExtras, RegionalIPCallExtensions

    names = [f.name for f in dataclasses.fields(RegionalIPCallExtensions)]
    assert tuple(names[-4:]) == pipeline.REGIONAL_IP_ARGUMENTS == ("ip_adapter_mask", "control_ip_adapter_image", "control_ip_adapter_image_embeds",
                                                                   "control_ip_adapter_scale")
    assert names[:-4] == [f.name for f in dataclasses.fields(LineCallExtensions)] and issubclass(RegionalIPCallExtensions, LineCallExtensions)
    d = RegionalIPCallExtensions()
    assert d.ip_adapter_mask is None and d.control_ip_adapter_image is None and d.control_ip_adapter_image_embeds is None and d.control_ip_adapter_scale == 1.0
    assert "regional_ip" in {f.name for f in dataclasses.fields(LoopExtras)} and LoopExtras().regional_ip is None
    # a call that names one of them carries the widest record (it may name line prompts too); every other call the record it always did
    pipe = _pipe()
    seen = []
    pipe.check_inputs = lambda *a, **k: seen.append(pipe._call_extensions)
    for kw in (dict(control_ip_adapter_scale=0.5, control_prompt=["x"]), dict(ip_adapter_mask="m"), dict(control_prompt=["x"]), dict(true_cfg_scale=2.0), {}):
        with pytest.raises(Exception):
            pipe(**dict(_kw(), prompt_embeds=None), **kw)
    assert seen == [RegionalIPCallExtensions(control_ip_adapter_scale=0.5, control_prompt=["x"]), RegionalIPCallExtensions(ip_adapter_mask="m"),
                    LineCallExtensions(control_prompt=["x"]), CallExtensions(true_cfg_scale=2.0), CallExtensions()]
    assert [type(s) for s in seen] == [RegionalIPCallExtensions, RegionalIPCallExtensions, LineCallExtensions, CallExtensions, CallExtensions]
    assert pipe._call_extensions is None


def test_row_weights_make_the_rows_call(monkeypatch):
    """ops.ip_attention_gated(row_weights=None) makes the native call it always made; with a table it calls rt_ip_attention_rows with the
    table and its batch stride (0: one table for the batch) after the gate's two arguments."""
    from reptext_amd import native, ops

    calls = []
    monkeypatch.setattr(native, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(ops, "_stream", lambda: 0x50)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    B, N, H, n = 2, 24, 2, 4
    d = H * 128
    qkv, wq = torch.zeros(B, N, 3 * d, dtype=torch.bfloat16), torch.zeros(128, dtype=torch.bfloat16)
    kv, out, gate = torch.zeros(1, n, 2 * d, dtype=torch.bfloat16), torch.zeros(B, N, d), torch.zeros(B, 6 * d)
    q, k, v, g = qkv[..., :d], kv[..., :d], kv[..., d:], gate[:, 2 * d : 3 * d]
    ops.ip_attention_gated(q, wq, k, v, out, H, 0.6, g, True, 0.11, 1e-5)
    ops.ip_attention_gated(q, wq, k, v, out, H, 0.6, g, True, 0.11, 1e-5, row_weights=None)
    assert calls[0] == calls[1] and calls[0][0] == "rt_ip_attention_gated" and len(calls[0][1]) == 23
    old = calls[0][1]
    shared, per = torch.zeros(1, N), torch.zeros(B, N + 8)[:, :N]
    for w, swb in ((shared, 0), (per, N + 8)):
        calls.clear()
        assert ops.ip_attention_gated(q, wq, k, v, out, H, 0.6, g, True, 0.11, 1e-5, row_weights=w) is out
        (name, a), = calls
        assert name == "rt_ip_attention_rows" and len(a) == len(native.SIGNATURES[name]) == 25
        assert a == old[:10] + (w.data_ptr(), swb) + old[10:]
    calls.clear()
    ops.ip_attention(q, wq, k, v, out, H, 0.6, row_weights=shared)
    assert calls[0][0] == "rt_ip_attention_rows" and calls[0][1][8:12] == (None, 0, shared.data_ptr(), 0)
    for bad in (torch.zeros(N), torch.zeros(3, N), torch.zeros(1, N + 1), torch.zeros(1, 2 * N)[:, ::2]):
        with pytest.raises(ValueError, match="row_weights must be"):
            ops.ip_attention_gated(q, wq, k, v, out, H, row_weights=bad)
    with pytest.raises(TypeError, match="float32"):
        ops.ip_attention_gated(q, wq, k, v, out, H, row_weights=shared.to(torch.bfloat16))
