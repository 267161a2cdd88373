"""LoRA adapters for the MMDiT models: diffusers/PEFT-format state dicts, the per-model adapter state, and the on-device merge.

The reference's pipeline is a ``FluxLoraLoaderMixin`` (PIPE:15,163) and its ControlNet a ``PeftAdapterMixin`` (CN:22,41) that scales
the LoRA layers per call from ``joint_attention_kwargs["scale"]`` (PIPE:908-925, CN:263-276). Here adapters are not separate layers:
every targeted bf16 weight holds

    W = bf16(W0 + Σ_{a fused} f_a·σ_a·B_a·A_a + [enabled]·Σ_{a active, not fused} s·w_a·σ_a·B_a·A_a),   σ_a = α_a / r_a

merged in place on the device (rt_lora_merge_bf16, one rounding) from a kept pristine copy W0, so the denoising loop and a captured
graph of it run the unchanged kernels on the same buffers at no per-step cost. The weight is a pure function of the adapter state and
the call scale s (1.0 outside a call): the manager keeps the term list it last applied to each module and re-merges, always from W0,
exactly the modules whose list changed. Term lists are ordered by adapter name and terms with a zero coefficient are dropped, so one
state gives one set of bits whatever sequence of calls reached it.

Outside a call the scale is 1.0 as far as ``state_dict()`` / ``save_pretrained()`` see it; the parameters themselves keep the last call's
scale until the next call or adapter change (re-merging after every call would double the merge passes of a scaled call).

Format rules (recalled from diffusers / PEFT; parity with them is unpinned, nothing can be checked offline):
  * keys ``[<prefix>.]<module path>.lora_A.weight`` [r, in] and ``.lora_B.weight`` [out, r]; module paths are the models'
    diffusers names (modules.Lin holders);
  * α: a per-module ``<path>.alpha`` scalar; else ``lora_alpha`` / ``r`` of the safetensors header's ``lora_adapter_metadata``
    JSON (keys with or without the ``<prefix>.`` prefix); else σ = 1;
  * a newly loaded adapter becomes the only active one, at weight 1.0;
  * factors are cast to bf16 (what the reference's bf16 pipeline holds);
  * unloading keeps fused adapters in the weights (``fuse_lora(); unload_lora_weights()`` bakes the adapter in).
Refused with a ValueError: kohya / BFL keys, text-encoder keys, DoRA, alpha_pattern / rank_pattern, unknown module paths, shape
mismatches, more than RT_LORA_MAX_TERMS terms on one module, in-features not a multiple of 8 (and, for the tower's hint embedder, of 64:
its K-padded copy is cached), a model that is not on the GPU.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from .native import RT_LORA_MAX_TERMS as MAX_TERMS
DEFAULT_WEIGHT_NAME = "pytorch_lora_weights.safetensors"
_SUFFIX_A, _SUFFIX_B, _SUFFIX_ALPHA = ".lora_A.weight", ".lora_B.weight", ".alpha"


def _first(keys, n: int = 3) -> str:
    keys = sorted(keys)
    return ", ".join(keys[:n]) + (f" (+{len(keys) - n} more)" if len(keys) > n else "")


def read_lora_file(path_or_dict, weight_name: Optional[str] = None) -> Tuple[Dict[str, torch.Tensor], Dict]:
    """(state dict, adapter metadata) from a dict, a ``.safetensors`` file, or a directory / local hub id (modules.resolve_model_path;
    nothing is fetched). In a directory: ``weight_name``, else pytorch_lora_weights.safetensors, else its only .safetensors file."""
    if isinstance(path_or_dict, dict):
        return dict(path_or_dict), {}
    path = str(path_or_dict)
    if not os.path.isfile(path):
        from .modules import resolve_model_path

        d = resolve_model_path(path)
        if weight_name is not None:
            path = os.path.join(d, weight_name)
        elif os.path.isfile(os.path.join(d, DEFAULT_WEIGHT_NAME)):
            path = os.path.join(d, DEFAULT_WEIGHT_NAME)
        else:
            files = sorted(f for f in os.listdir(d) if f.endswith(".safetensors"))
            if len(files) != 1:
                raise ValueError(f"{d}: pass weight_name= ({len(files)} .safetensors files and no {DEFAULT_WEIGHT_NAME})")
            path = os.path.join(d, files[0])
        if not os.path.isfile(path):
            raise OSError(f"LoRA file {path} not found")
    if not path.endswith(".safetensors"):
        raise ValueError(f"{path}: only .safetensors LoRA files are read")
    from safetensors import safe_open

    with safe_open(path, framework="pt") as f:
        meta = f.metadata() or {}
        sd = {k: f.get_tensor(k) for k in f.keys()}
    raw = meta.get("lora_adapter_metadata")
    return sd, (json.loads(raw) if raw else {})


def parse_lora_state_dict(sd: Dict[str, torch.Tensor], metadata: Optional[Dict] = None, prefix: str = "transformer"):
    """{module path: (A [r, in], B [out, r], σ)} of a diffusers/PEFT LoRA state dict; refuses the formats this path does not read."""
    keys = list(sd)
    bad = [k for k in keys if k.startswith("lora_unet_") or "lora_down" in k or "lora_up" in k]
    if bad:
        raise ValueError(f"kohya/BFL-format LoRA keys are not supported (convert to the diffusers/PEFT format first): {_first(bad)}")
    bad = [k for k in keys if k.startswith(("text_encoder.", "text_encoder_2."))]
    if bad:
        raise ValueError(f"LoRA on the text encoders is not supported: {_first(bad)}")
    bad = [k for k in keys if "lora_magnitude_vector" in k]
    if bad:
        raise ValueError(f"DoRA adapters are not supported: {_first(bad)}")
    meta = {}
    for k, v in (metadata or {}).items():
        meta[k[len(prefix) + 1:] if k.startswith(prefix + ".") else k] = v
    bad = [k for k in ("alpha_pattern", "rank_pattern") if meta.get(k)]
    if bad:
        raise ValueError(f"LoRA metadata with {', '.join(bad)} is not supported")
    parts: Dict[str, Dict[str, torch.Tensor]] = {}
    unknown = []
    for k, v in sd.items():
        p = k[len(prefix) + 1:] if k.startswith(prefix + ".") else k
        for suf, slot in ((_SUFFIX_A, "A"), (_SUFFIX_B, "B"), (_SUFFIX_ALPHA, "alpha")):
            if p.endswith(suf):
                parts.setdefault(p[: -len(suf)], {})[slot] = v
                break
        else:
            unknown.append(k)
    if unknown:
        raise ValueError(f"unrecognised LoRA keys (expected <module>.lora_A.weight / .lora_B.weight / .alpha): {_first(unknown)}")
    meta_sigma = None
    if meta.get("lora_alpha") is not None and meta.get("r"):
        meta_sigma = float(meta["lora_alpha"]) / float(meta["r"])
    out = {}
    for path, d in parts.items():
        if "A" not in d or "B" not in d:
            raise ValueError(f"LoRA module '{path}' lacks its {'lora_A' if 'A' not in d else 'lora_B'} weight")
        A, B = d["A"], d["B"]
        if A.dim() != 2 or B.dim() != 2 or A.shape[0] != B.shape[1]:
            raise ValueError(f"LoRA module '{path}': lora_A {tuple(A.shape)} and lora_B {tuple(B.shape)} do not form a rank-r pair")
        r = A.shape[0]
        if "alpha" in d:
            sigma = float(d["alpha"].reshape(-1)[0]) / r
        else:
            sigma = meta_sigma if meta_sigma is not None else 1.0
        out[path] = (A, B, sigma)
    return out


@dataclass
class Factor:
    """One adapter's factors for one module: B [out, r_pad], At = Aᵀ [in, r_pad] (bf16, zero columns r..), σ = α / r."""

    B: torch.Tensor
    At: torch.Tensor
    r: int
    sigma: float


def pad_factors(A: torch.Tensor, B: torch.Tensor, sigma: float, device) -> Factor:
    r = A.shape[0]
    r_pad = (r + 31) // 32 * 32
    Bp = torch.zeros(B.shape[0], r_pad, dtype=torch.bfloat16, device=device)
    At = torch.zeros(A.shape[1], r_pad, dtype=torch.bfloat16, device=device)
    Bp[:, :r] = B.to(torch.bfloat16).to(device)
    At[:, :r] = A.to(torch.bfloat16).t().to(device)
    return Factor(Bp, At, r, float(sigma))


def _names(x) -> List[str]:
    return [x] if isinstance(x, str) else list(x)


class LoraState:
    """The adapter state of one model (pure Python): loaded adapters, the active list with weights, the enabled flag and the fused
    coefficients. ``terms(s)`` gives every targeted module's (adapter, coefficient) list at call scale s."""

    def __init__(self):
        self.adapters: Dict[str, Dict[str, Factor]] = {}
        self.active: List[Tuple[str, float]] = []
        self.enabled = True
        self.fused: Dict[str, float] = {}

    def _check_names(self, names):
        missing = [n for n in names if n not in self.adapters]
        if missing:
            raise ValueError(f"unknown adapter(s) {missing}; loaded: {sorted(self.adapters)}")

    def _contributing(self) -> List[Tuple[str, Optional[float]]]:
        """(adapter, fused coefficient or None = active unfused term) in name order."""
        act = dict(self.active)
        out = []
        for a in sorted(self.adapters):
            if a in self.fused:
                out.append((a, self.fused[a]))
            elif self.enabled and a in act:
                out.append((a, None))
        return out

    def terms(self, s: float = 1.0) -> Dict[str, List[Tuple[str, float]]]:
        act = dict(self.active)
        out: Dict[str, List[Tuple[str, float]]] = {}
        for a, f in self._contributing():
            k = f if f is not None else s * act[a]
            for path, fac in self.adapters[a].items():
                c = k * fac.sigma
                if c != 0.0:
                    out.setdefault(path, []).append((a, c))
        return out

    def _apply_checked(self, change) -> None:
        """Apply ``change`` only if no module ends up with more than MAX_TERMS terms (else the state is left as it was)."""
        saved = (dict(self.adapters), list(self.active), self.enabled, dict(self.fused))
        change()
        counts: Dict[str, int] = {}
        for a, _ in self._contributing():
            for p in self.adapters[a]:
                counts[p] = counts.get(p, 0) + 1
        over = [p for p, n in counts.items() if n > MAX_TERMS]
        if over:
            self.adapters, self.active, self.enabled, self.fused = saved
            raise ValueError(f"more than {MAX_TERMS} simultaneous LoRA terms on module(s) {_first(over)}")

    def add(self, name: str, factors: Dict[str, Factor]) -> None:
        if name in self.adapters:
            raise ValueError(f"adapter '{name}' is already loaded")

        def ch():
            self.adapters[name] = factors
            self.active = [(name, 1.0)]
        self._apply_checked(ch)

    def set_adapters(self, names, weights=None) -> None:
        names = _names(names)
        self._check_names(names)
        if weights is None or isinstance(weights, (int, float)):
            weights = [1.0 if weights is None else float(weights)] * len(names)
        weights = [1.0 if w is None else float(w) for w in weights]
        if len(weights) != len(names):
            raise ValueError(f"{len(names)} adapter names but {len(weights)} weights")
        self._apply_checked(lambda: setattr(self, "active", list(zip(names, weights))))

    def fuse(self, lora_scale: float = 1.0, names=None) -> None:
        act = dict(self.active)
        names = [a for a, _ in self.active] if names is None else _names(names)
        self._check_names(names)
        again = [n for n in names if n in self.fused]
        if again:
            raise ValueError(f"adapter(s) {again} are already fused; unfuse_lora() first")

        def ch():
            for n in names:
                self.fused[n] = float(lora_scale) * act.get(n, 1.0)
        self._apply_checked(ch)

    def unfuse(self) -> None:
        self.fused = {}

    def delete(self, names) -> None:
        names = _names(names)
        self._check_names(names)
        for n in names:
            self.adapters.pop(n)
            self.fused.pop(n, None)
        self.active = [(a, w) for a, w in self.active if a not in names]

    def set_enabled(self, on: bool) -> None:
        self._apply_checked(lambda: setattr(self, "enabled", bool(on)))


class LoraManager:
    """LoraState of one model plus its device side: the W0 copies (per module, taken on first use), the term list last applied to
    each module, and the merge of the modules whose list changed. fp8 plans (enable_fp8_linears) get the merged rows requantised
    into their existing e4m3 / scale tensors (per-output-channel scales: rows are independent), so plans and captured graphs stay
    valid."""

    def __init__(self, model):
        self.state = LoraState()
        self.w0: Dict[str, torch.Tensor] = {}
        self.applied: Dict[str, Tuple[Tuple[str, float], ...]] = {}
        self._model = model

    def load(self, name: str, parsed) -> None:
        """Check ``parse_lora_state_dict`` output against the model and add it as adapter ``name`` (no merge yet)."""
        from .modules import Lin

        m = self._model
        mods = dict(m.named_modules())
        unknown = [p for p in parsed if not isinstance(mods.get(p), Lin)]
        if unknown:
            raise ValueError(f"LoRA targets unknown module path(s) of {type(m).__name__}: {_first(unknown)}")
        for p, (A, B, _) in sorted(parsed.items()):
            lin = mods[p]
            if A.shape[1] != lin.in_features or B.shape[0] != lin.out_features:
                raise ValueError(f"LoRA module '{p}': lora_A {tuple(A.shape)} / lora_B {tuple(B.shape)} do not match the Linear "
                                 f"[{lin.out_features}, {lin.in_features}]")
            why = m._lora_unsupported(p, lin)
            if why:
                raise ValueError(f"LoRA module '{p}': {why} (not supported)")
        if m.device.type != "cuda":
            raise ValueError(f"{type(m).__name__} is on {m.device}: LoRA adapters are merged on the GPU (there is no CPU fallback); "
                             "move the model to the GPU first")
        self.state.add(name, {p: pad_factors(A, B, sigma, m.device) for p, (A, B, sigma) in sorted(parsed.items())})

    def sync(self, s: float = 1.0) -> int:
        """Bring every targeted weight to the state at call scale s, on the current stream; returns the number of modules merged."""
        want = self.state.terms(s)
        changed = sorted(p for p in set(want) | set(self.applied) if tuple(want.get(p, ())) != self.applied.get(p, ()))
        if not changed:
            return 0
        from . import ops

        fp8 = self._model._fp8_rows()
        for p in changed:
            w = self._model.get_submodule(p).weight.data
            if p not in self.w0:
                self.w0[p] = w.clone()
            terms = [(self.state.adapters[a][p].B, self.state.adapters[a][p].At, c) for a, c in want.get(p, ())]
            ops.lora_merge_(w, self.w0[p], terms)
            if p in fp8:
                full, w8, ws, r0, r1 = fp8[p]
                ops.quantize_rows_fp8_into(full[r0:r1][None], w8[r0:r1][None], ws[r0:r1])
            self.applied[p] = tuple(want.get(p, ()))
        return len(changed)

    def unload(self) -> None:
        """diffusers' unload_lora_weights: the adapters go, what is FUSED stays in the weights (parity unpinned). Every weight becomes
        bf16(W0 + its fused terms), bit for bit W0 when nothing is fused; unfused adapters, W0 copies and factors are dropped with the
        manager."""
        keep = LoraState()
        keep.adapters = {a: f for a, f in self.state.adapters.items() if a in self.state.fused}
        keep.fused = dict(self.state.fused)
        self.state = keep
        self.sync()

    def to_device(self, device) -> None:
        self.w0 = {p: t.to(device) for p, t in self.w0.items()}
        for mods in self.state.adapters.values():
            for f in mods.values():
                f.B, f.At = f.B.to(device), f.At.to(device)
