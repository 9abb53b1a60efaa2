#!/usr/bin/env python3
"""Innermost-loop report for one kernel of a .hip file (gfx950 assembly).

Compiles the file device-only to assembly (no GPU needed), finds the named
kernel, and for every loop the compiler marks in its block comments (the
innermost ones, and the own blocks of loops that hold others) prints

  * its length in instructions,
  * an opcode histogram,
  * the memory timeline: the position of every global_load and of every
    s_waitcnt vmcnt(N) in the loop body, so one can read off how many loads
    are in flight when a wait retires which of them.

    python tools/isa_loops.py es_pytorch_amd/ops/csrc/hip/rollout_loco.hip \
        loco_pair_step_fp8_kernel [--min-len 40] [-D NAME=VALUE]

With --summary it prints, for every kernel whose name holds the given string
(each instantiation of a template), the memory instructions by segment (flat,
global, scratch, ds) and the histogram of s_waitcnt forms.

It is a reading aid: it reports ordinary opcodes and checks nothing.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

_INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)\b(.*)$")
_VMCNT = re.compile(r"vmcnt\((\d+)\)")


def compile_asm(src, flags, arch="gfx950"):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = [hipcc, f"--offload-arch={arch}", "-O3", "-std=c++17", "-S",
               "--cuda-device-only", *flags, src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{r.stderr[-4000:]}")
        with open(out) as f:
            return f.read().splitlines()


def kernel_body(lines, kernel):
    """Lines of the first function whose (mangled) label contains `kernel`."""
    start = None
    for n, ln in enumerate(lines):
        if start is None:
            if re.match(r"^[A-Za-z_]\w*:", ln) and kernel in ln.split(":")[0]:
                start = n
        elif ln.startswith(".Lfunc_end"):
            return lines[start:n]
    raise SystemExit(f"kernel {kernel!r} not found")


def resources(lines, kernel):
    """The compiler's resource comment lines that follow the kernel."""
    out, on = {}, False
    for ln in lines:
        if re.match(r"^[A-Za-z_]\w*:", ln):
            on = kernel in ln.split(":")[0]
        if on:
            m = re.match(r"^; (NumVgprs|NumAgprs|ScratchSize|Occupancy|"
                         r"LDSByteSize|SGPRBlocks|NumSgprs): (\S+)", ln)
            if m:
                out.setdefault(m.group(1), m.group(2))
    return out


_BLOCK = re.compile(r"^(?:\.L|; %bb\.)(?:BB)?(\d+_\d+|\d+):")
_HEADER = re.compile(r"=>\s*This (Inner )?Loop Header: Depth=(\d+)")
_MEMBER = re.compile(r"in Loop: Header=BB(\d+_\d+) Depth=(\d+)")


def loops(body):
    """{header: (depth, inner, [(first_line, last_line)])} from the block
    comments the compiler writes: a loop's own blocks are its header block and
    every block marked 'in Loop: Header=<it>' (blocks of a nested loop name
    the nested header and are counted there, not here)."""
    starts = [n for n, ln in enumerate(body) if _BLOCK.match(ln)]
    out, order = {}, []
    for j, n in enumerate(starts):
        end = (starts[j + 1] if j + 1 < len(starts) else len(body)) - 1
        ln = body[n]
        for nxt in body[n + 1:end + 1]:  # the comment may run over lines
            if not nxt.lstrip().startswith(";"):
                break
            ln += nxt
        h = _HEADER.search(ln)
        m = _MEMBER.search(ln)
        if h:
            name = re.match(r"^\.LBB(\d+_\d+):", ln).group(1)
            out[name] = [int(h.group(2)), bool(h.group(1)), [(n, end)]]
            order.append(name)
        elif m and m.group(1) in out:
            out[m.group(1)][2].append((n, end))
    return [(k, *out[k]) for k in order]


def insns(body, spans):
    out = []
    for lo, hi in spans:
        for ln in body[lo:hi + 1]:
            if ln.lstrip().startswith((";", ".")):
                continue
            m = _INSN.match(ln)
            if m:
                out.append((m.group(1), m.group(2)))
    return out


def report(name, depth, inner, ins, top):
    hist = collections.Counter(op for op, _ in ins)
    kind = "innermost" if inner else "has nested loops, own blocks only"
    print(f"loop .LBB{name} (depth {depth}, {kind}): {len(ins)} instructions")
    items = hist.most_common(top)
    for k in range(0, len(items), 4):
        print("   " + "  ".join(f"{op:>22s} {c:3d}" for op, c in items[k:k + 4]))
    rest = sum(hist.values()) - sum(c for _, c in items)
    if rest:
        print(f"   (+{rest} in {len(hist) - len(items)} other opcodes)")
    tl, run, nload = [], 0, 0
    for pos, (op, rest_) in enumerate(ins):
        if op.startswith("global_load"):
            if not run:
                tl.append([pos, 0])
            tl[-1][1] += 1
            run = 1
            nload += 1
            continue
        run = 0
        if op == "s_waitcnt":
            m = _VMCNT.search(rest_)
            if m:
                tl.append(f"@{pos} vmcnt({m.group(1)})")
    line = "  ".join(f"@{t[0]} load x{t[1]}" if isinstance(t, list) else t
                     for t in tl)
    print(f"   global_load {nload}; timeline: {line or '-'}")


_SEGMENTS = ("flat", "global", "scratch", "ds")
_WAIT_ARG = re.compile(r"(vmcnt|lgkmcnt|expcnt)\((\d+)\)")


def kernel_names(lines, kernel):
    """Mangled labels of every function whose name contains `kernel`."""
    return [ln.split(":")[0] for ln in lines
            if re.match(r"^[A-Za-z_]\w*:", ln) and kernel in ln.split(":")[0]]


def summary(body):
    """(memory instructions by segment, histogram of s_waitcnt forms) of one
    kernel: {segment: Counter(opcode)}, Counter('vmcnt(3) lgkmcnt(0)')."""
    mem = {s: collections.Counter() for s in _SEGMENTS}
    waits = collections.Counter()
    for op, rest in insns(body, [(0, len(body) - 1)]):
        seg = op.split("_", 1)[0]
        if seg in mem and "_" in op:
            mem[seg][op] += 1
        elif op == "s_waitcnt":
            form = " ".join(f"{k}({n})" for k, n in _WAIT_ARG.findall(rest))
            waits[form or rest.strip()] += 1
    return mem, waits


def report_summary(label, body):
    mem, waits = summary(body)
    print(f"{label}:")
    for seg in _SEGMENTS:
        ops = ", ".join(f"{op} {c}" for op, c in sorted(mem[seg].items()))
        print(f"   {seg:8s}{sum(mem[seg].values()):5d}  {ops}")
    vm = collections.Counter()
    for form, c in waits.items():
        m = _VMCNT.search(form)
        if m:
            vm["vmcnt(0)" if m.group(1) == "0" else "vmcnt(n>0)"] += c
    print(f"   s_waitcnt {sum(waits.values())}: " +
          "  ".join(f"{k} {c}" for k, c in sorted(vm.items())))
    for form, c in sorted(waits.items(), key=lambda kv: (-kv[1], kv[0])):
        print(f"   {c:5d}  {form}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("src")
    ap.add_argument("kernel")
    ap.add_argument("--min-len", type=int, default=0,
                    help="hide loops shorter than this many instructions")
    ap.add_argument("--top", type=int, default=16, help="histogram rows")
    ap.add_argument("-D", dest="defs", action="append", default=[],
                    help="preprocessor definition passed to hipcc, e.g. -D NDEBUG=1")
    ap.add_argument("--has", default="",
                    help="only loops holding an opcode with this prefix")
    ap.add_argument("--summary", action="store_true",
                    help="for every kernel whose name holds KERNEL: memory "
                         "instructions by segment (flat, global, scratch, ds) and "
                         "the histogram of s_waitcnt forms, instead of the loops")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    a = ap.parse_args()
    if a.asm:
        with open(a.asm) as f:
            lines = f.read().splitlines()
    else:
        lines = compile_asm(a.src, [f"-D{d}" for d in a.defs])
    if a.summary:
        for name in kernel_names(lines, a.kernel):
            res = resources(lines, name)
            report_summary(name + "  " + "  ".join(f"{k}={v}" for k, v in res.items()),
                           kernel_body(lines, name))
        return
    res = resources(lines, a.kernel)
    print(f"{a.kernel}: " + "  ".join(f"{k}={v}" for k, v in res.items()))
    body = kernel_body(lines, a.kernel)
    for name, depth, inner, spans in loops(body):
        ins = insns(body, spans)
        if len(ins) >= a.min_len and (not a.has or any(op.startswith(a.has) for op, _ in ins)):
            report(name, depth, inner, ins, a.top)


if __name__ == "__main__":
    sys.exit(main())
