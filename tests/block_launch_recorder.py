"""What tests/test_block_launches_host.py records: the native calls that mmdit's plan_double / plan_single / run_double / run_single make
for one double and one single block, on the host, with CPU tensors standing in for device ones. A plain helper module, not a test file.

native.call is replaced by a recorder, native.load by a stub that answers the two size queries, ops._stream by a constant and
torch.Tensor.is_cuda by True. Every argument is decoded through the header's own signature (native.SIGNATURES): a pointer becomes
"<buffer>+<byte offset>", an array of structs one {field=value} group per element with its zero and null fields left out.
Buffers are named without reference to any plan field or workspace attribute:
  a block parameter      by its named_parameters() name ("double.attn.to_q.weight"), found through its storage (after a plan has fused
                         q|k|v, the parameter at the start of the fused storage names it);
  an e4m3 weight copy    "e4m3(<parameter>)" and its scales "scales(<parameter>)": the outputs of the plan-time rt_quantize_rows_fp8
                         call on that parameter;
  every other buffer     "b<k>", k = the order of its first appearance in the stream.
mmdit is touched only through plan_double, plan_single, Workspace, run_double, run_single (and the FUSED_QK_ROPE switch)."""
import contextlib
import ctypes as C
import json
import os

import torch

BF16, F32 = torch.bfloat16, torch.float32
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "block_launches.json")
STREAM = 0x5EED
B, T, N = 2, 64, 128          # two images (the per-image loops run twice), T % 64 == 0 (the MX row offset rule)


class _Lib:
    """Stands in for the loaded library: the two size queries that the block path makes."""

    @staticmethod
    def rt_attention_ws_bytes(B, S, H):
        return 0

    @staticmethod
    def rt_attention_fp8_vt_bytes(B, S, H):
        return B * H * 128 * ((S + 127) // 128 * 128)


class Recorder:
    def __init__(self):
        self.lines = []
        self.blocks = {}          # prefix -> module whose parameters name their storages
        self.tracked = []         # tensors allocated while recording, kept alive so that no address comes back
        self.copies = {}          # storage address -> name, for the plan-time e4m3 copies and their scales
        self.order = {}           # storage address -> "b<k>"

    def track(self, t):
        self.tracked.append(t)
        return t

    def new(self, *shape, dtype=BF16):
        return self.track(torch.zeros(*shape, dtype=dtype))

    def _extent(self, ptr):
        """(name or None, storage address, byte offset) of the buffer that holds ptr."""
        for prefix, blk in self.blocks.items():
            for p in blk.parameters():
                st = p.data.untyped_storage()
                if st.data_ptr() <= ptr < st.data_ptr() + st.nbytes():
                    first = next(n for n, q in blk.named_parameters() if q.data.data_ptr() == st.data_ptr())
                    return f"{prefix}.{first}", st.data_ptr(), ptr - st.data_ptr()
        for t in self.tracked:
            st = t.untyped_storage()
            if st.data_ptr() <= ptr < st.data_ptr() + st.nbytes():
                return None, st.data_ptr(), ptr - st.data_ptr()
        raise AssertionError(f"pointer {ptr:#x} lies in no parameter and no buffer allocated while recording")

    def pointer(self, ptr):
        if ptr is None:
            return "null"
        if ptr == STREAM:
            return "stream"
        name, base, off = self._extent(ptr)
        if name is None:
            name = self.copies.get(base) or self.order.setdefault(base, f"b{len(self.order)}")
        return f"{name}+{off}"

    def _struct(self, s):
        out = []
        for field, ctype in s._fields_:
            v = getattr(s, field)
            if ctype is C.c_void_p:
                if v is not None:
                    out.append(f"{field}={self.pointer(v)}")
            elif v != 0:
                out.append(f"{field}={v!r}")
        return "{" + " ".join(out) + "}"

    def call(self, name, *args):
        from reptext_amd import native

        sig = native.SIGNATURES[name]
        assert len(args) == len(sig), f"{name}: {len(args)} arguments for {len(sig)} parameters"
        if name == "rt_quantize_rows_fp8":                       # (x, ldx, x_f32, q, ldq, scales, rows, D, stream)
            src, _, off = self._extent(args[0])
            if src is not None and off == 0:                      # a whole parameter: the plan-time copy of a weight
                self.copies[self._extent(args[3])[1]] = f"e4m3({src})"
                self.copies[self._extent(args[5])[1]] = f"scales({src})"
        out = []
        for a, ctype in zip(args, sig):
            if ctype is C.c_void_p:
                out.append(self.pointer(a))
            elif isinstance(a, C.Array):
                out.append("[" + " ".join(self._struct(s) for s in a) + "]")
            else:
                out.append(repr(a))
        self.lines.append(f"{name}({', '.join(out)})")


@contextlib.contextmanager
def recording(rec, fused_qk_rope=True):
    from reptext_amd import mmdit, native, ops

    empty = torch.empty
    saved = [(native, "call", native.call), (native, "load", native.load), (ops, "_stream", ops._stream), (torch, "empty", torch.empty),
             (mmdit, "FUSED_QK_ROPE", mmdit.FUSED_QK_ROPE)]
    native.call, native.load, ops._stream = rec.call, lambda: _Lib, lambda: STREAM
    torch.empty = lambda *a, **kw: rec.track(empty(*a, **kw))
    torch.Tensor.is_cuda = property(lambda self: True)          # shadows the base class's attribute; deleted again below
    mmdit.FUSED_QK_ROPE = fused_qk_rope
    try:
        yield rec
    finally:
        del torch.Tensor.is_cuda
        for obj, attr, value in saved:
            setattr(obj, attr, value)


# mode -> settings. level: the fp8 argument of plan_*; attn8: fp8_attention; ip: None | "xlabs" (double block only) | "instantx" (both);
# inject: a sample added by the double block; single_inject: by the single block; mods: adaLN vectors given instead of temb.
MODES = {}
for _level in (False, "ln", "all", "mx"):
    for _attn8 in (False, True):
        MODES[f"{_level or 'bf16'}{'+attn8' if _attn8 else ''}"] = dict(level=_level, attn8=_attn8)
MODES.update({
    "bf16 xlabs": dict(ip="xlabs"),
    "bf16 xlabs+inject": dict(ip="xlabs", inject=True),
    "bf16 instantx": dict(ip="instantx"),
    "all+attn8 xlabs+inject": dict(level="all", attn8=True, ip="xlabs", inject=True),
    "all+attn8 instantx": dict(level="all", attn8=True, ip="instantx"),
    "mx xlabs+inject": dict(level="mx", ip="xlabs", inject=True),
    "mx instantx": dict(level="mx", ip="instantx"),
    "mx+attn8 xlabs+inject": dict(level="mx", attn8=True, ip="xlabs", inject=True),
    "mx+attn8 instantx": dict(level="mx", attn8=True, ip="instantx"),
    "bf16 single inject": dict(single_inject=True),
    "mx single inject": dict(level="mx", single_inject=True),
    "bf16 mods": dict(mods=True),
    "bf16 window": dict(window=(16, 48)),
    "bf16 unfused qk rope": dict(fused_qk_rope=False),
    "bf16 d128": dict(H=1),
    "all d128": dict(H=1, level="all"),
})


def blocks(H):
    from reptext_amd.modules import DoubleBlockParams, SingleBlockParams

    d = H * 128
    return DoubleBlockParams(d, 128, dtype=BF16), SingleBlockParams(d, 128, dtype=BF16)


def record(level=False, attn8=False, ip=None, inject=False, single_inject=False, mods=False, window=None, fused_qk_rope=True, H=2):
    """The launch stream of one mode, plan-time launches included: a list of lines."""
    from reptext_amd import mmdit

    rec = Recorder()
    d, S = H * 128, T + N
    with recording(rec, fused_qk_rope):
        dbl, sgl = blocks(H)
        rec.blocks = {"double": dbl, "single": sgl}
        pd = mmdit.plan_double(dbl, fp8=level, fp8_attention=attn8)
        ps = mmdit.plan_single(sgl, fp8=level, fp8_attention=attn8)
        ws = mmdit.Workspace(B, T, N, d, torch.device("cpu"), True)
        temb, cos, sin = rec.new(B, d, dtype=F32), rec.new(S, 128, dtype=F32), rec.new(S, 128, dtype=F32)
        table = rec.new(3 * B, 15 * d, dtype=F32)[B : 2 * B]          # one step's rows of a table: [image 6d | text 6d | single 3d]
        kv = rec.new(B, 4, 2 * d)
        adapter = (kv[..., :d], kv[..., d:], 0.6)
        sample = rec.new(B, N, d)
        mmdit.run_double(pd, ws, None if mods else temb, cos, sin, H, inject=sample if inject else None,
                         mods=(table[:, : 6 * d], table[:, 6 * d : 12 * d]) if mods else None, ip=adapter if ip else None,
                         ip_inside=ip == "instantx", window=window)
        mmdit.run_single(ps, ws, None if mods else temb, cos, sin, H, inject=sample if single_inject else None,
                         mods=table[:, 12 * d :] if mods else None, ip=adapter if ip == "instantx" else None)
    return rec.lines


def record_all():
    return {mode: record(**kw) for mode, kw in MODES.items()}


if __name__ == "__main__":        # how the fixture was written, once, from the tree before the projections were folded
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(FIXTURE, "w") as f:
        json.dump(record_all(), f, indent=0)
        f.write("\n")
