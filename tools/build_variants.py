#!/usr/bin/env python3
"""Cross-compile control kernel libraries for same-box A/B runs.

Builds one _hip_ops .so from the kernel sources of each given git revision
(checked out into a temp tree) into es_pytorch_amd/ops/variants/
(gitignored), e.g. the parent commit as the control arm of alternated runs:

    python tools/build_variants.py --revs HEAD~1

Then, on the GPU box, alternate the tree's own library with the control:

    python tools/kbench.py --pair --graph --steps 1000
    ES_HIP_SO=es_pytorch_amd/ops/variants/hip_HEADp1.so \
        python tools/kbench.py --pair --graph --steps 1000
"""
import argparse
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from es_pytorch_amd import ops  # noqa: E402

VAR_DIR = os.path.join(os.path.dirname(ops.__file__), "variants")


def build_rev_control(rev: str) -> str:
    """Compile the kernel sources as they were at `rev` (control arm)."""
    os.makedirs(VAR_DIR, exist_ok=True)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.path.join(VAR_DIR, f"hip_{rev.replace('~', 'p').replace('/', '_')}.so")
    with tempfile.TemporaryDirectory() as td:
        subprocess.run(["git", "archive", rev, "es_pytorch_amd/ops/csrc"],
                       cwd=repo, check=True,
                       stdout=open(os.path.join(td, "a.tar"), "wb"))
        subprocess.run(["tar", "xf", "a.tar"], cwd=td, check=True)
        d = os.path.join(td, "es_pytorch_amd", "ops", "csrc", "hip")
        srcs = sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith(".hip"))
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared",
               "-fPIC", *srcs, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
    print("built", out, f"(sources @ {rev})")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--revs", nargs="+", required=True,
                    help="git revisions to build as control arms")
    a = ap.parse_args()
    for rev in a.revs:
        build_rev_control(rev)
