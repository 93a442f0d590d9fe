#!/usr/bin/env python3
"""Resource usage of the kernels of one .hip file (device assembly metadata): VGPRs, spilled VGPRs, scratch bytes per lane, LDS,
the waves per SIMD the registers allow (512 VGPRs per SIMD lane, allocated in blocks of 8, at most 8 waves), the workgroups per CU
the LDS allows (160 KiB per CU) and the static count of vector-ALU instructions in the kernel's body.
    python tools/kernel_resources.py me_frame.hip [name pattern] [extra hipcc flags...]
Fails (exit status 1, the compiler's messages on stderr) when hipcc fails, when the assembly holds no kernel metadata or when no
kernel matches the pattern."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svt-av1-mod-by-patman_amd", "csrc")
LDS_PER_CU, VGPRS_PER_LANE, VGPR_BLOCK, MAX_WAVES = 160 * 1024, 512, 8, 8


def fail(msg):
    print("kernel_resources.py: " + msg, file=sys.stderr)
    sys.exit(1)


def static_valu(asm, symbol):
    """vector-ALU instructions between the kernel's label and the end of its body (.Lfunc_end)"""
    m = re.search(r"^" + re.escape(symbol) + r":[^\n]*\n(.*?)^\.Lfunc_end", asm, re.S | re.M)
    if not m:
        return "?"
    return str(sum(1 for ln in m.group(1).split("\n") if re.match(r"\s+v_", ln)))


def main():
    if len(sys.argv) < 2:
        fail("usage: kernel_resources.py FILE.hip [name pattern] [extra hipcc flags...]")
    src = sys.argv[1]
    pat = sys.argv[2] if len(sys.argv) > 2 else ""
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "--cuda-device-only", "-S",
           "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, src), "-o", "-"] + sys.argv[3:]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=CSRC)
    if r.returncode != 0:
        fail(f"hipcc exited with {r.returncode}:\n{r.stderr[-4000:]}")
    out = r.stdout
    at = out.rfind("amdhsa.kernels:")
    if at < 0:
        fail(f"no kernel metadata in the assembly of {src}")
    shown = 0
    for blk in re.split(r"\n  - \.agpr_count", out[at:])[1:]:
        blk = ".agpr_count" + blk
        g = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1]  # noqa: E731
        name = g("name")
        dem = subprocess.run(["c++filt", name], stdout=subprocess.PIPE, text=True).stdout.strip()
        if pat not in dem:
            continue
        dem = re.sub(r"^(void )?(\(anonymous namespace\)::)?", "", dem).split("(")[0]   # a template kernel's name carries its return type
        try:
            regs = int(g("vgpr_count"))  # arch + accumulation registers of the unified file
            alloc = max(VGPR_BLOCK, (regs + VGPR_BLOCK - 1) // VGPR_BLOCK * VGPR_BLOCK)
            waves = str(min(MAX_WAVES, VGPRS_PER_LANE // alloc))
            lds = int(g("group_segment_fixed_size"))
            wgs = str(LDS_PER_CU // lds) if lds else "-"
        except ValueError:
            waves = wgs = "?"
        print(f"{dem[:44]:44s} vgpr {g('vgpr_count'):>4s} spill {g('vgpr_spill_count'):>3s} scratch {g('private_segment_fixed_size'):>4s} B  "
              f"lds {g('group_segment_fixed_size'):>6s} B  sgpr {g('sgpr_count'):>3s}  waves/SIMD {waves}  lds wg/CU {wgs:>3s}  "
              f"static VALU {static_valu(out, name):>5s}")
        shown += 1
    if not shown:
        fail(f"no kernel of {src} matches '{pat}'")


if __name__ == "__main__":
    main()
