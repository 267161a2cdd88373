"""Host side of the path a call's extension arguments take: the one record (``CallExtensions``) and the one decorator that leaves it on
the pipeline while the call runs, the loop's extras that ``_denoise`` takes as an argument, and the one rule for doubling a tensor under
CFG. CPU-constructed tiny models; no kernel runs here."""
import dataclasses
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ip_adapter_reference as ipr  # noqa: E402
from test_true_cfg_host import _kw, _pipe, assert_no_call_state  # noqa: E402
from test_union_tower_host import SMALL_T, call_kwargs, make_pipe  # noqa: E402

DEFAULTS = dict(ip_adapter_image=None, ip_adapter_image_embeds=None,
                control_image_union=None, controlnet_conditioning_scale_union=1.0, control_guidance_start_union=0.0,
                control_guidance_end_union=1.0,
                negative_prompt=None, negative_prompt_2=None, true_cfg_scale=1.0, negative_prompt_embeds=None,
                negative_pooled_prompt_embeds=None, negative_ip_adapter_image=None, negative_ip_adapter_image_embeds=None)


def test_the_record_has_the_thirteen_keywords_and_their_defaults():
    from reptext_amd import pipeline
    from reptext_amd.pipeline import CallExtensions, FluxControlNetPipeline
    from reptext_amd.pipeline_inpaint import FluxControlNetPipeline as InpaintPipeline

    fields = dataclasses.fields(CallExtensions)
    assert [f.name for f in fields] == list(DEFAULTS) and len(fields) == 13
    assert {f.name: f.default for f in fields} == DEFAULTS and dataclasses.asdict(CallExtensions()) == DEFAULTS
    assert all(type(f.default) is type(DEFAULTS[f.name]) for f in fields)                 # 1.0 and not 1
    assert tuple(f.name for f in fields[6:]) == pipeline.TRUE_CFG_ARGUMENTS
    # no keyword that a pipeline takes as an extension is a parameter of its __call__: the base pipeline takes all 13, the inpaint
    # pipeline the IP-Adapter's two (four of the negative prompt's names are parameters of the reference's inpaint __call__ itself)
    base, inpaint = (set(inspect.signature(cls.__call__).parameters) for cls in (FluxControlNetPipeline, InpaintPipeline))
    assert not set(DEFAULTS) & base
    assert set(DEFAULTS) & inpaint == {"negative_prompt", "negative_prompt_2", "negative_prompt_embeds", "negative_pooled_prompt_embeds"}
    for name in set(DEFAULTS) - inpaint - {"ip_adapter_image", "ip_adapter_image_embeds"}:
        with pytest.raises(TypeError, match=name):                                        # not taken off: Python's own error names it
            _pipe(inpaint=True)(**_kw(), **{name: DEFAULTS[name]})


def test_the_record_is_on_the_pipeline_during_the_call_and_never_after(monkeypatch):
    from reptext_amd.pipeline import CallExtensions

    pipe = _pipe()
    assert pipe._call_extensions is None
    seen = []
    check_inputs = pipe.check_inputs
    monkeypatch.setattr(pipe, "check_inputs", lambda *a, **k: (seen.append(pipe._call_extensions), check_inputs(*a, **k))[1])
    with pytest.raises(ValueError, match="divisible by 8"):                               # raised by check_inputs
        pipe(**dict(_kw(), height=65), true_cfg_scale=3.0, negative_prompt="blurry", control_guidance_end_union=0.5)
    assert seen == [CallExtensions(true_cfg_scale=3.0, negative_prompt="blurry", control_guidance_end_union=0.5)]      # as passed, no more
    assert pipe._call_extensions is None
    for bad, name in ((dict(negative_prompt=7), "negative_prompt"),                       # raised by the extension checks
                      (dict(control_image_union=torch.zeros(1, 16, 64)), "control_image_union"),
                      (dict(ip_adapter_image_embeds=torch.zeros(1, 1, 32)), "no IP-Adapter is loaded")):
        with pytest.raises(ValueError, match=name):
            pipe(**_kw(), **bad)
        assert pipe._call_extensions is None
    with pytest.raises(TypeError, match="no_such_keyword"):
        pipe(**_kw(), no_such_keyword=1)
    assert pipe._call_extensions is None
    inp = _pipe(inpaint=True)
    with pytest.raises(ValueError, match="IP-Adapter"):
        inp(**_kw(), ip_adapter_image=object())
    assert inp._call_extensions is None
    assert_no_call_state(pipe), assert_no_call_state(inp)


def test_a_direct_denoise_sees_nothing_of_an_earlier_call():
    """One call with an image prompt, a union tower and true CFG together, then ``_denoise`` with its 15 positional arguments, the way
    the benchmark makes it: the loop of the second gets plain extras, by construction and not because something was cleared."""
    from reptext_amd.pipeline import LoopExtras, UnionTower

    pipe = make_pipe()
    pipe.load_ip_adapter(ipr.init_ip_params(SMALL_T, n_tokens=4, embed_dim=32, seed=6))
    seen = []

    def recorder(latents, *args, **kwargs):
        seen.append((args, kwargs))
        pipe._master_latents = latents
        return latents

    pipe._denoise_eager = recorder
    bf16 = torch.bfloat16
    hint = torch.ones(1, 16, 64, dtype=bf16)
    out = pipe(**call_kwargs(control_image_union=hint, controlnet_conditioning_scale_union=0.7, control_guidance_end_union=0.5,
                             ip_adapter_image_embeds=torch.ones(1, 1, 32), true_cfg_scale=2.0,
                             negative_prompt_embeds=torch.ones(1, 8, 64, dtype=bf16), negative_pooled_prompt_embeds=torch.ones(1, 32, dtype=bf16)))
    assert out.images.shape == (1, 16, 64) and len(seen) == 1
    args, kwargs = seen[0]
    assert len(args) == 15 and list(kwargs) == ["extras"]                                 # 16 positional parameters and the one keyword
    x = kwargs["extras"]
    assert isinstance(x, LoopExtras) and x.cfg_scale == 2.0 and x.extra_towers == () and x.velocity is None and x.quiet is False
    assert x.ip_embeds.shape == (2, 32) and x.ip_embeds.dtype == bf16 and x.ip_embeds.tolist() == [[0.0] * 32, [1.0] * 32]     # negative first
    assert isinstance(x.union, UnionTower) and x.union.model is pipe.controlnet_union and x.union.scale == 0.7 and x.union.active_steps == (0,)
    assert x.union.hint.shape == (2, 16, 64)                                              # a [1,N,C] hint at total == 1 is doubled
    assert args[0].shape == (2, 8, 64) and pipe._call_extensions is None                  # prompt_embeds: [negative, positive]

    lat, pe, pooled = torch.zeros(1, 16, 64, dtype=bf16), torch.zeros(1, 8, 64, dtype=bf16), torch.zeros(1, 32, dtype=bf16)
    timesteps = torch.tensor([1000.0, 500.0])
    got = pipe._denoise(lat, pe, pooled, torch.zeros(8, 3), torch.zeros(16, 3), timesteps, [], [], 3.5, 1.0, 2, None, None, [], 2)
    assert got is lat and len(seen) == 2
    args, kwargs = seen[1]
    x = kwargs["extras"]
    assert len(args) == 15 and list(kwargs) == ["extras"]
    assert x.ip_embeds is None and x.union is None and x.cfg_scale is None and x.extra_towers == () and x.velocity is None
    assert x == LoopExtras()


# What the parent commit's five sites did, read off them: the text-line hints (_collect_hints), the union hint and the inpaint hint
# doubled `if cfg and shape[0] == total`, the masks of both pipelines `if cfg and shape[0] == total and total > 1`.
# (mask?, batch of the tensor, total) -> batch without CFG, batch under CFG
DOUBLING = {(False, 1, 1): (1, 2),      # a [1,N,C] hint at total == 1 counts as per-image: doubled
            (False, 1, 2): (1, 1),      # a shared hint serves both halves
            (False, 2, 2): (2, 4),
            (True, 1, 1): (1, 1),       # [1,N,1] means "shared" for a mask, also at total == 1
            (True, 1, 2): (1, 1),
            (True, 2, 2): (2, 4)}


@pytest.mark.parametrize("mask, batch, total", list(DOUBLING), ids=lambda v: str(v))
def test_one_rule_doubles_hints_and_masks_under_cfg(mask, batch, total):
    from reptext_amd.pipeline import FluxControlNetPipeline
    from reptext_amd.pipeline_inpaint import FluxControlNetPipeline as InpaintPipeline

    assert InpaintPipeline._doubled_under_cfg is FluxControlNetPipeline._doubled_under_cfg
    t = torch.arange(batch * 16 * (1 if mask else 128), dtype=torch.float32).reshape(batch, 16, -1)
    for cfg, want in zip((False, True), DOUBLING[(mask, batch, total)]):
        out = FluxControlNetPipeline._doubled_under_cfg(t, total, cfg, mask=mask)
        assert out.shape == (want,) + t.shape[1:]
        assert out is t if want == batch else torch.equal(out, torch.cat([t, t]))
        if not mask:                                                                      # and through the site of the text-line hints
            hints, _, _ = make_pipe(union=None)._collect_hints([t], None, 64, 64, total, 1, "cpu", torch.float32, cfg=cfg)
            assert len(hints) == 1 and hints[0].shape == out.shape
