"""Timing-only ablation builds of csrc/attention.hip (results wrong by construction). The switches live HERE, not in the product
kernel: this script re-inserts them into a generated copy (tools/attn_dev/attention_abl.hip, git-ignored) and builds one harness
binary per variant:  python tools/attn_dev/make_ablations.py [VARIANT ...]   (variants: NOSOFT NOEXP NOLDS NODMA NOCOMBINE EXP_NOWEAVE)
The front end in attention.hip offers every launch to csrc/attention_v3.hip first, which is linked in unpatched: run the binaries
with RT_ATTN_V3=0 to time this kernel at shapes attention_v3 would take."""
import os, subprocess, sys
here = os.path.dirname(os.path.abspath(__file__))
root = os.path.dirname(os.path.dirname(here))
csrc = os.path.join(root, "arabic-text-image-generation-reptext_amd", "csrc")
s = open(os.path.join(csrc, "attention.hip")).read()
PAIRS = [('#pragma unroll\n      for (int j = 0; j < 8; ++j) {\n        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[8 * s2 + j], scale_log2, -m_run));\n        ps += p;\n        pf[j] = (__bf16)p;\n      }\n', '#ifdef ATT_ABL_NOSOFT\n      pf = __builtin_bit_cast(bf16x8, f32x4{s[8 * s2], s[8 * s2 + 1], s[8 * s2 + 2], s[8 * s2 + 3]});\n      ps = s[8 * s2 + 4];\n#else\n#pragma unroll\n      for (int j = 0; j < 8; ++j) {\n#ifdef ATT_ABL_NOEXP\n        const float p = __builtin_fmaf(s[8 * s2 + j], scale_log2, -m_run);\n#else\n        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[8 * s2 + j], scale_log2, -m_run));\n#endif\n        ps += p;\n        pf[j] = (__bf16)p;\n      }\n#endif\n'), ('#define RT_WEAVE(n, nds, nva)   ', '#ifdef ATT_EXP_NOWEAVE\n#define RT_WEAVE(n, nds, nva)\n#else\n#define RT_WEAVE(n, nds, nva)   '), ('    if ((nva) > 0) __builtin_amdgcn_sched_group_barrier(0x402, (nva), 0); \\\n  }\n', '    if ((nva) > 0) __builtin_amdgcn_sched_group_barrier(0x402, (nva), 0); \\\n  }\n#endif\n'), ('      auto kread = [&](int h, int ks) -> bf16x8 {\n        return', '      auto kread = [&](int h, int ks) -> bf16x8 {\n#ifdef ATT_ABL_NOLDS\n        return qf[(ks + h) & 7];\n#endif\n        return'), ('      auto vread = [&](int h, int s2, int dt) -> bf16x8 {\n', '      auto vread = [&](int h, int s2, int dt) -> bf16x8 {\n#ifdef ATT_ABL_NOLDS\n        return qf[(dt + 2 * s2 + h) & 7];\n#endif\n'), ('      f32x16 s0, s1;\n', '#ifdef ATT_EXP_PRIO\n      __builtin_amdgcn_s_setprio(ATT_EXP_PRIO);\n#endif\n      f32x16 s0, s1;\n'), ('      if (RT_RARE(t + 1 < te && next_ragged)) stage(SLOT ^ 1, t + 1, true);', '#ifndef ATT_ABL_NODMA\n      if (RT_RARE(t + 1 < te && next_ragged)) stage(SLOT ^ 1, t + 1, true);\n#endif\n     '), ('      const bool weave = t + 1 < te && !next_ragged;\n', '#ifdef ATT_ABL_NODMA\n      const bool weave = false;\n#else\n      const bool weave = t + 1 < te && !next_ragged;\n#endif\n'), ('    if (!whole) {\n      // ---- partial', '#ifdef ATT_ABL_NOCOMBINE\n    if (!whole) continue;\n#endif\n    if (!whole) {\n      // ---- partial')]
for product, ablated in PAIRS:
    assert s.count(product) == 1, product[:60]
    s = s.replace(product, ablated)
open(os.path.join(here, "attention_abl.hip"), "w").write(s)
v3o = os.path.join(here, "attention_v3.o")
cmd = (f"hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-honor-nans -fno-slp-vectorize -mllvm -amdgpu-spill-vgpr-to-agpr=0 -I{root}/include -I{csrc} "
       f"-c {csrc}/attention_v3.hip -o {v3o}")
print(cmd, flush=True)
subprocess.run(cmd, shell=True, check=True)
for v in (sys.argv[1:] or ["BASE", "NOSOFT", "NOEXP", "NOLDS", "NODMA", "NOCOMBINE"]):
    flag = "" if v == "BASE" else ("-DATT_" + ("" if v.startswith("EXP_") else "ABL_") + v)
    cmd = f"hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-honor-nans -I{root}/include -I{csrc} {flag} {here}/attention_abl.hip {csrc}/version.hip {here}/main.cpp -Xlinker {v3o} -o {here}/attn_v_{v}"
    print(cmd, flush=True)
    subprocess.run(cmd, shell=True, check=True)
