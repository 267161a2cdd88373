"""The protocol every record of ``LoopExtras`` has for the captured denoise loop — its part of the graph key (``signature``), its static
inputs by name (``tensors``) and itself on the graph's clones (``rebound``) — and the walk ``LoopExtras`` makes over them. The expected
key is written out from the stanzas ``_denoise`` had before the records took them over: element for element, flat where they were flat.
CPU tensors, a stub ``sig`` / ``ident`` / adapter; no kernel runs."""
import dataclasses
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_union_tower_host import make_pipe  # noqa: E402

from reptext_amd.guidance import Guidance, TrueCFGGuider  # noqa: E402
from reptext_amd.pipeline import LinePrompts, LoopExtras, RegionalIP, Repaint, UnionTower  # noqa: E402

sig = lambda t: ("sig", tuple(t.shape), str(t.dtype))
ident = lambda m: ("ident", m)
ADAPTER = SimpleNamespace(version=7, scales=[0.5, 0.25])
MODEL = "the union model"
z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype)        # every tensor below has a shape of its own

IPE, HINT = z(2, 32), z(2, 16, 64)
SRC, NOISE, MASK = z(1, 16, 61), z(1, 16, 62), z(1, 16, 63)
L_EMB, L_VIS = z(2, 128, 48), z(2, 208, dtype=torch.int32)
R_EMB, R_IMG, R_TXT = (z(1, 33), z(2, 34)), (None, z(2, 16)), (None, z(2))
GUIDER = TrueCFGGuider(start=0.0, stop=0.5, eta=0, norm_threshold=2, momentum=-0.5)

FIELDS = dict(ip_embeds=IPE, union=UnionTower(MODEL, HINT, 0.7, (0, 2)), cfg_scale=2.5, repaint=Repaint(SRC, NOISE, MASK),
              guidance=Guidance(GUIDER, (0, 1)), line_prompts=LinePrompts(L_EMB, (64, 128, 192, 208), L_VIS),
              regional_ip=RegionalIP(R_EMB, R_IMG, R_TXT))
# what each field added to the key, in the order of the stanzas
KEY = dict(ip_embeds=(sig(IPE), 7, (0.5, 0.25)),
           union=("union", ident(MODEL), sig(HINT), 0.7, (0, 2)),
           cfg_scale=(("cfg", 2.5),),
           repaint=(("repaint", sig(SRC), sig(NOISE), sig(MASK)),),
           guidance=(("guidance", (0, 1), 0.0, 2.0, -0.5),),
           line_prompts=(("line_prompts", (64, 128, 192, 208), sig(L_VIS), sig(L_EMB)),),
           regional_ip=(("regional_ip", 2, (False, True), (sig(R_EMB[0]), sig(R_EMB[1])), (None, sig(R_IMG[1]))), 7, (0.5, 0.25)))
TENSORS = dict(ip_embeds=IPE, union_hint=HINT, repaint_src=SRC, repaint_noise=NOISE, repaint_mask=MASK, line_embeds=L_EMB, line_row_vis=L_VIS,
               rip_embeds0=R_EMB[0], rip_embeds1=R_EMB[1], rip_img_w1=R_IMG[1], rip_txt_w1=R_TXT[1])


def test_the_key_of_a_call_with_every_extension_is_the_stanzas_in_their_order():
    assert list(FIELDS) == list(KEY) == [f.name for f in dataclasses.fields(LoopExtras) if f.name in KEY]       # field order = key order
    got = LoopExtras(**FIELDS).signature(sig, ident, ADAPTER)
    assert got == sum(KEY.values(), ()) and len(got) == 3 + 5 + 1 + 1 + 1 + 1 + 3
    assert [type(x) for x in got[9:12]] == [tuple] * 3 and all(type(x) is float for x in got[10][2:])      # ints of the guider as floats
    # the records' own methods: what LoopExtras walks
    assert FIELDS["union"].signature(sig, ident) == KEY["union"]
    assert FIELDS["repaint"].signature(sig) == KEY["repaint"] and FIELDS["line_prompts"].signature(sig) == KEY["line_prompts"]
    assert FIELDS["guidance"].signature() == KEY["guidance"] and (FIELDS["regional_ip"].signature(sig),) == KEY["regional_ip"][:1]


@pytest.mark.parametrize("name", list(KEY))
def test_a_field_alone_adds_its_own_slice_and_an_absent_one_nothing(name):
    assert LoopExtras().signature(sig, ident, ADAPTER) == () and LoopExtras().signature(sig, ident, None) == ()
    assert LoopExtras(**{name: FIELDS[name]}).signature(sig, ident, ADAPTER) == KEY[name]
    rest = {k: v for k, v in FIELDS.items() if k != name}
    assert LoopExtras(**rest).signature(sig, ident, ADAPTER) == sum((KEY[k] for k in rest), ())
    # what is no extension of the captured loop adds nothing either
    assert LoopExtras(tower_window=(3, 9), extra_towers=((MODEL, HINT, 1.0),), velocity=max, quiet=True).signature(sig, ident, ADAPTER) == ()


def test_the_static_inputs_are_the_records_own_tensors_under_their_names():
    got = LoopExtras(**FIELDS).tensors()
    assert list(got) == list(TENSORS) and all(got[k] is TENSORS[k] for k in TENSORS)
    # the walk finds a record by its ``tensors`` method, not by a list of names: every field that holds tensors is walked or is ip_embeds
    walked = [k for k, v in FIELDS.items() if hasattr(v, "tensors")]
    assert walked == ["union", "repaint", "line_prompts", "regional_ip"] and all(hasattr(v, "tensors") == hasattr(v, "rebound") for v in FIELDS.values())
    assert all(list(LoopExtras(**{k: FIELDS[k]}).tensors()) == list(FIELDS[k].tensors()) != [] for k in walked)
    assert LoopExtras().tensors() == {} and LoopExtras(cfg_scale=2.5, guidance=FIELDS["guidance"]).tensors() == {}
    assert list(LoopExtras(repaint=FIELDS["repaint"], ip_embeds=IPE).tensors()) == ["ip_embeds", "repaint_src", "repaint_noise", "repaint_mask"]
    assert list(FIELDS["union"].tensors()) == ["union_hint"] and list(FIELDS["line_prompts"].tensors()) == ["line_embeds", "line_row_vis"]


def test_rebound_extras_hold_the_clones_and_nothing_else_changes():
    rest = dict(tower_window=(3, 9), extra_towers=((MODEL, HINT, 1.0),), velocity=max)
    extras = LoopExtras(**FIELDS, **rest)
    static = {name: t.clone() for name, t in extras.tensors().items()}
    static.update(latents=z(1, 16, 64), hints=[z(1, 16, 128)])                 # the graph's base inputs are in the same dict
    bound = extras.rebound(static)
    got = bound.tensors()
    assert list(got) == list(TENSORS) and all(got[k] is static[k] and got[k] is not TENSORS[k] for k in TENSORS)
    assert bound.quiet is True and extras.quiet is False
    assert bound.cfg_scale == 2.5 and bound.guidance is extras.guidance and all(getattr(bound, k) == v for k, v in rest.items())
    assert bound.union.model is MODEL and bound.union.scale == 0.7 and bound.union.active_steps == (0, 2)
    assert bound.line_prompts.ends == (64, 128, 192, 208) and bound.regional_ip.img_w[0] is None and bound.regional_ip.txt_w[0] is None
    assert bound.signature(sig, ident, ADAPTER) == extras.signature(sig, ident, ADAPTER)            # a capture runs under the key it is filed under
    # absent fields stay absent
    plain = LoopExtras(cfg_scale=2.5, **rest).rebound(dict(latents=z(1, 16, 64)))
    assert plain == LoopExtras(cfg_scale=2.5, quiet=True, **rest)
    one = LoopExtras(repaint=FIELDS["repaint"]).rebound({k: v.clone() for k, v in FIELDS["repaint"].tensors().items()})
    assert all(getattr(one, k) is None for k in KEY if k != "repaint") and one.repaint.src32 is not SRC


def test_what_a_graph_keeps_alive_besides_its_inputs():
    plans, pad = object(), object()
    union = UnionTower(SimpleNamespace(_ensure_plans=lambda: plans, _cx_pad=pad), HINT, 1.0, (0,))
    tr = SimpleNamespace(_ip_adapter=ADAPTER)
    assert LoopExtras().kept(tr) == [None] and LoopExtras(union=union).kept(SimpleNamespace()) == [None, plans, pad]
    assert LoopExtras(ip_embeds=IPE).kept(tr) == [ADAPTER] and LoopExtras(regional_ip=FIELDS["regional_ip"], union=union).kept(tr) == [ADAPTER, plans, pad]


@pytest.mark.parametrize("fails", [True, False])
def test_a_capture_leaves_the_host_state_it_found_and_a_failed_one_cleans_up(monkeypatch, capsys, fails):
    """``_capture_loop`` with the graph API and the models' plans stubbed (nothing runs on a device): during the capture both modules
    record into one keep list; after it, failed or not, the scheduler's step index and history length are what they were and
    ``CAPTURE_KEEP`` is cleared; a failure also drops the attention workspaces that appeared, withdraws the sample buffers' window
    promise, says so on stderr and returns "failed"."""
    from reptext_amd import mmdit, ops
    from reptext_amd.pipeline import _SampleCache
    from reptext_amd.scheduler import FlowMatchMultistepScheduler

    class Capture:
        def __init__(self, graph, capture_error_mode=None):
            assert capture_error_mode == "thread_local"

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    synced = []
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda: "graph")
    monkeypatch.setattr(torch.cuda, "graph", Capture)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: synced.append(1))
    monkeypatch.setattr(ops, "_ATTN_WS", {"before": 1})
    pipe = make_pipe()
    for m in (pipe.transformer, pipe.controlnet):
        m._ensure_plans = lambda: "plans"
    pipe.scheduler = FlowMatchMultistepScheduler()
    pipe.scheduler._step_index, pipe.scheduler._history_len = 5, 0
    pipe._sample_cache = _SampleCache(("key",), [], [], window=(0, 4))
    pipe._sample_promise = (0, 4)
    lat = z(1, 4, 64)
    ins = dict(latents=lat, hints=[HINT], ip_embeds=IPE)

    def loop(named, extras):
        assert mmdit.CAPTURE_KEEP is ops.CAPTURE_KEEP and ops.CAPTURE_KEEP[:4] == ["plans", "plans", getattr(pipe.controlnet, "_cx_pad", None), None]
        assert list(named) == list(ins) and named["latents"] is not lat and named["hints"][0] is not HINT and extras.quiet
        assert extras.ip_embeds is named["ip_embeds"] and extras.ip_embeds is not IPE
        pipe.scheduler._step_index, pipe.scheduler._history_len = 9, 1             # what the loop's steps do to the scheduler
        ops._ATTN_WS["during"] = 2
        pipe._master_latents = "out32"
        if fails:
            raise RuntimeError("boom")
        return "out"

    ent = pipe._capture_loop(ins, LoopExtras(ip_embeds=IPE), loop)
    assert (pipe.scheduler._step_index, pipe.scheduler._history_len) == (5, 0) and mmdit.CAPTURE_KEEP is None and ops.CAPTURE_KEEP is None
    err = capsys.readouterr().err
    if fails:
        assert ent == "failed" and synced == [1] and ops._ATTN_WS == {"before": 1} and pipe._sample_cache.window is None
        assert err == "[reptext_amd] hipGraph capture of the denoise loop failed (RuntimeError: boom); staying eager\n"
    else:
        assert err == "" and not synced and ops._ATTN_WS == {"before": 1, "during": 2} and pipe._sample_cache.window == (0, 4)
        assert {k: ent[k] for k in ("graph", "out", "out32", "window")} == dict(graph="graph", out="out", out32="out32", window=(0, 4))
        assert ent["samples"] is pipe._sample_cache and ent["samples"] in ent["keep"] and list(ent["static"]) == list(ins)


def test_the_sample_cache_has_field_names_and_a_plain_promise():
    from reptext_amd.pipeline import FluxControlNetPipeline, _SampleCache

    bufs = [torch.ones(1, 4, 2), torch.ones(1, 4, 2)]
    cache = _SampleCache(("key",), bufs, [torch.ones(1, 4, 2)])
    assert [f.name for f in dataclasses.fields(cache)] == ["key", "double", "single", "window"] and cache.window is None
    FluxControlNetPipeline._zero_samples_for(None, (0, 2))                              # no tower: nothing to promise
    FluxControlNetPipeline._zero_samples_for(cache, None)                               # the full path: no fill
    assert cache.window is None and all(bool((b == 1).all()) for b in bufs)
    FluxControlNetPipeline._zero_samples_for(cache, (0, 2))                             # a window is set: zeroed once
    assert cache.window == (0, 2) and all(bool((b == 0).all()) for b in bufs) and bool((cache.single[0] == 1).all())
    bufs[0].fill_(3.0)
    FluxControlNetPipeline._zero_samples_for(cache, (0, 2))                             # the same window: the promise holds, no fill
    assert bool((bufs[0] == 3).all())
    FluxControlNetPipeline._zero_samples_for(cache, (1, 3))
    assert cache.window == (1, 3) and bool((bufs[0] == 0).all())
