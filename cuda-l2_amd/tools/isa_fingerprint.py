"""Per-kernel fingerprints of the device code (gfx950 ISA as hipcc -S prints it), so a later change to the sources can show
which kernels' instruction streams it touched -- and therefore which committed measurements still describe the library.

    python tools/isa_fingerprint.py [--csrc DIR --include DIR] > profiles/<name>.json        (no GPU; ~20 s, one hipcc per unit in parallel)
    python tools/isa_fingerprint.py --units 13 > profiles/sq_one_isa_fingerprint.json         (the one-tile kernel's unit)
    python tools/isa_fingerprint.py --units 0 1 2 3 13 --opt -O2 --flag=-DHGEMM_TIMELINE      (another build of the same sources)

A kernel's fingerprint is the sha256 of its function body between the label and s_endpgm with comments, assembler directives
and basic-block label NUMBERS stripped (labels are numbered per translation unit: adding a kernel renumbers them all).
tests/test_build_audit.py compares units 0-3 of the current sources with profiles/r0{4,5,6}_isa_fingerprint_*_library.json,
tests/test_sq_one_build.py unit 13 with profiles/sq_one_isa_fingerprint.json.
"""
import argparse
import hashlib
import json
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

PKG = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
DEFAULT_UNITS = (0, 1, 2, 3)


def compile_groups(csrc: Path, include: Path, opt: str = "-O3", units=DEFAULT_UNITS, flags=()) -> str:
    """hipcc -S --cuda-device-only of the instantiation units hgemm_inst_g<unit>.hip (the flags of tests/test_build_audit.py, plus
    `flags`); returns the text."""
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for grp in units:
            out = Path(tmp) / f"g{grp}.s"
            procs.append((out, subprocess.Popen([HIPCC, "--offload-arch=gfx950", opt, "-std=c++17", *flags, f"-I{csrc}", f"-I{include}", "-S", "--cuda-device-only",
                                                 str(csrc / f"hgemm_inst_g{grp}.hip"), "-o", str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)))
        text = ""
        for out, pr in procs:
            _, err = pr.communicate(timeout=900)
            if pr.returncode != 0:
                raise RuntimeError(err.decode()[-2000:])
            text += out.read_text()
    return text


def kernel_bodies(text: str) -> dict:
    out = {}
    for m in re.finditer(r"^(_ZN12hgemm_mi355x\w+):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M):
        body = re.sub(r";.*", "", m.group(2))
        body = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", body)
        out[m.group(1)] = "\n".join(ln.rstrip() for ln in body.splitlines() if ln.strip() and not ln.strip().startswith("."))
    return out


def fingerprints(text: str) -> dict:
    return {k: hashlib.sha256(v.encode()).hexdigest()[:20] for k, v in sorted(kernel_bodies(text).items())}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--csrc", default=str(PKG / "csrc"))
    ap.add_argument("--include", default=str(PKG.parent / "include"))
    ap.add_argument("--note", default="")
    ap.add_argument("--units", type=int, nargs="+", default=list(DEFAULT_UNITS), help="instantiation units hgemm_inst_g<N>.hip (default: 0 1 2 3)")
    ap.add_argument("--opt", default="-O3", help="optimisation level (default: -O3)")
    ap.add_argument("--flag", action="append", default=[], help="extra compiler flag, repeatable: --flag=-DHGEMM_TIMELINE")
    a = ap.parse_args()
    fp = fingerprints(compile_groups(Path(a.csrc), Path(a.include), a.opt, a.units, a.flag))
    units = "{" + ",".join(str(u) for u in a.units) + "}" if a.units != list(DEFAULT_UNITS) else "{0..3}"
    flags = " ".join(["hipcc --offload-arch=gfx950", a.opt, "-std=c++17", *a.flag, "-S --cuda-device-only", f"hgemm_inst_g{units}.hip"])
    json.dump({"note": a.note, "flags": flags, "kernels": fp}, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
