#!/usr/bin/env python3
"""Per-kernel register / scratch / occupancy table of a kernel source file (hipcc
-Rpass-analysis=kernel-resource-usage), e.g.  python tools/resource_usage.py encode_encrypt [-D...]
From Python: table("encode_encrypt") returns the rows (tests/build_support.py reads them)."""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table(name, extra_flags=(), timeout=1200):
    """Compile kernels/<name>.hip for gfx950 and return one dict per kernel, in the compiler's order: "kernel" (the
    demangled name without its argument list and "void seamd::") plus every field of the remark ("VGPRs", "AGPRs",
    "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]", ...) as the compiler's string.
    A compile that fails gives no remarks, hence []."""
    csrc = os.path.join(ROOT, "seal-embedded_amd", "csrc")
    with tempfile.TemporaryDirectory(prefix="ru_") as tmp:
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950",
               "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-c", os.path.join(csrc, "kernels", name + ".hip"),
               "-o", os.path.join(tmp, name + ".o"), "-Rpass-analysis=kernel-resource-usage"] + list(extra_flags)
        err = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout).stderr
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark: [^:]*:\d+:\d+: +(.*?) \[-Rpass", line) or re.search(r"remark: +(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            full = subprocess.run(["c++filt", t.split(":", 1)[1].strip()], capture_output=True, text=True).stdout.strip()
            cur = {"kernel": re.sub(r"\(.*", "", full).replace("void seamd::", "")}
            rows.append(cur)
        elif cur is not None and ":" in t:
            k, v = t.split(":", 1)
            cur[k.strip()] = v.strip()
    return rows


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "encode_encrypt"
    print("%-70s %5s %5s %8s %4s %7s" % ("kernel", "VGPR", "AGPR", "scratch", "occ", "LDS"))
    for r in table(name, sys.argv[2:], timeout=None):
        print("%-70s %5s %5s %8s %4s %7s" % (r["kernel"][:70], r.get("VGPRs", "?"), r.get("AGPRs", "?"),
                                            r.get("ScratchSize [bytes/lane]", "?"), r.get("Occupancy [waves/SIMD]", "?"),
                                            r.get("LDS Size [bytes/block]", "?")))


if __name__ == "__main__":
    main()
