#!/usr/bin/env python3
"""What the compiler made of the vector sections between the frontend's GEMMs (no GPU needed):
    hipcc -O3 -std=c++17 -I include --offload-arch=gfx950 --cuda-device-only -S silero_vad_amd/csrc/kernel_front_f43.hip -o f43.s
    python tools/asm_sections.py f43.s [symbol substring, default ILi32EfLi1E = 16 kHz float]
Prints the kernel's code size, registers and spills, its v_mov count, the histogram of VALU run lengths between two MFMAs (a "run" is
the code between two consecutive v_mfma, whatever else lies in it), and for every long run that is not an FFT pass -- the part
epilogues, the fold, the sections of encoders 1-3 -- its VALU, ds_read_b128 and s_waitcnt counts (profiles/r08a_front_sections.md)."""
import collections
import re
import sys

path = sys.argv[1]
want = sys.argv[2] if len(sys.argv) > 2 else "ILi32EfLi1E"
lines = open(path).read().splitlines()
start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*front_f43_kernel" + want + r"\S*:", l))
end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
body = [l.split(";")[0].strip() for l in lines[start + 1:end]]
ins = [l for l in body if l and not l.startswith(".") and not l.endswith(":")]
meta = {}
for l in lines[end:]:
    m = re.match(r"^; (codeLenInByte|NumVgprs|ScratchSize) *[:=] *(\d+)", l.strip())
    if m and m.group(1) not in meta:
        meta[m.group(1)] = int(m.group(2))
    if len(meta) == 3:
        break
op = [l.split()[0] for l in ins]
is_valu = lambda o: o.startswith("v_") and not o.startswith("v_mfma")
print(f"{want}: code {meta.get('codeLenInByte')} bytes, {meta.get('NumVgprs')} VGPRs, scratch {meta.get('ScratchSize')} bytes; "
      f"{len(ins)} instructions, {sum(o.startswith('v_mfma') for o in op)} v_mfma, {sum(map(is_valu, op))} VALU, "
      f"{sum(o.startswith('v_mov') or o.startswith('v_accvgpr') for o in op)} v_mov, {op.count('s_waitcnt')} s_waitcnt, "
      f"{op.count('ds_read_b128')} ds_read_b128")
runs, cur = [], collections.Counter()
for o in op:
    if o.startswith("v_mfma"):
        runs.append(cur)
        cur = collections.Counter()
    else:
        cur["valu"] += is_valu(o)
        cur[o] += 1
runs.append(cur)
hist = collections.Counter(r["valu"] for r in runs[1:-1] if r["valu"])
print("VALU runs between two MFMAs (length: how many):", ", ".join(f"{k}: {v}" for k, v in sorted(hist.items()) if k < 32))
print("long runs (VALU >= 32) that hold no ds_bpermute (not an FFT pass):")
for n, r in enumerate(runs):
    if r["valu"] >= 32 and not r["ds_bpermute_b32"]:
        cnt = lambda *pre: sum(v for k, v in r.items() if k.startswith(pre))
        print(f"  run {n:4d}: VALU {r['valu']:4d} (fma {cnt('v_fma', 'v_pk_fma')}, add/sub {cnt('v_add_f32', 'v_sub', 'v_pk_add')}, max {cnt('v_max', 'v_pk_max')}, "
              f"mov {cnt('v_mov', 'v_accvgpr')})  "
              f"ds_read_b128 {r['ds_read_b128']:3d}  s_waitcnt {r['s_waitcnt']:3d}  s_barrier {r['s_barrier']}")
