#!/usr/bin/env python3
"""Register table of the attention kernels, from the compiler's resource-usage remarks.

    python tools/attn_regs.py [--arch gfx950] [--all] [file.hip ...]

Compiles csrc/attention16.hip and csrc/attention.hip (device code only, nothing is linked or kept) with
-Rpass-analysis=kernel-resource-usage and prints, per kernel instantiation: VGPRs, AGPRs, scratch bytes per lane,
waves per SIMD and LDS bytes.  Exit status 1 if any listed kernel has scratch.  profiles/attn_vgpr_ab.txt holds the
table before and after the per-instantiation occupancy bounds.
"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "biggan-tensorflow_amd", "csrc")
FIELDS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "waves"), ("LDS Size [bytes/block]", "lds"), ("SGPRs", "sgpr"))


def kernel_name(mangled):
    """attn16_fwd_kernel<1, 2> from the Itanium name (no demangler needed: the template arguments are integers)"""
    if not mangled.startswith("_Z"):
        return mangled
    pos, name = 2 + (mangled[2:3] == "N"), None
    while True:
        m = re.match(r"L?(\d+)", mangled[pos:])
        if not m:
            break
        pos += m.end()
        name = mangled[pos:pos + int(m.group(1))]
        pos += int(m.group(1))
    if name is None:
        return mangled
    m = re.match(r"I((?:L[a-z]\d+E)+)E", mangled[pos:])
    args = re.findall(r"L[a-z](\d+)E", m.group(1)) if m else []
    return name + ("<" + ", ".join(args) + ">" if args else "")


def remarks(path, arch, hipcc):
    cmd = [hipcc, "--offload-arch=" + arch, "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", os.devnull,
           "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"), path]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr)
        raise SystemExit("compile failed: " + " ".join(cmd))
    rows, cur = [], None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            rows.append(cur)
            continue
        if cur is None or "remark:" not in line:
            continue
        for label, key in FIELDS:
            m = re.search(r"remark:\s+(?:Total)?" + re.escape(label) + r": (\d+)", line)
            if m:
                cur[key] = int(m.group(1))
                break
    for r in rows:
        r["name"] = kernel_name(r["name"])
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("files", nargs="*", default=[os.path.join(CSRC, "attention16.hip"), os.path.join(CSRC, "attention.hip")])
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "hipcc"))
    ap.add_argument("--all", action="store_true", help="every kernel of the files, not only attn*")
    a = ap.parse_args()
    bad = 0
    for path in a.files:
        print("# " + os.path.relpath(path, ROOT))
        print("%-44s %5s %5s %8s %6s %7s" % ("kernel", "VGPR", "AGPR", "scratch", "waves", "LDS"))
        for r in sorted(remarks(path, a.arch, a.hipcc), key=lambda r: r["name"]):
            if not a.all and not r["name"].startswith("attn"):
                continue
            print("%-44s %5d %5d %8d %6d %7d" % (r["name"], r.get("vgpr", -1), r.get("agpr", -1), r.get("scratch", -1),
                                                r.get("waves", -1), r.get("lds", -1)))
            bad += r.get("scratch", 0) > 0
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
