#!/usr/bin/env python3
"""Instructions one walk step issues, counted from the assembly `make asm` writes.

Usage: python tools/step_count.py [FILE.s] [--kernel REGEX] [--json]

For each kernel whose symbol matches REGEX (default: the three production
instantiations of trace_simple) it finds

  lockstep  the innermost loop that holds two `buffer_load_dwordx4 ... offen`
  solo      the innermost loop that holds an `s_load_dwordx8`

and prints, per loop, the instruction counts by class along the internal-node
path: once round the loop from its header, where a forward branch over a
region is taken when the region holds a load or 16 or more vector
instructions (a leaf's further loads, the triangle test) and some of the
loop's marker loads lie outside it, and is not taken otherwise (bookkeeping
that a step with lanes still walking runs).  Next to it: the whole loop's
counts and its scratch accesses.

Classes, by mnemonic prefix only: VALU `v_`; SMEM `s_load` / `s_buffer_load`;
branches `s_branch` / `s_cbranch`; waits `s_waitcnt` / `s_nop` / `s_sleep`;
SALU every other `s_`; VMEM `buffer_` / `global_` / `flat_` / `scratch_`;
anything else (LDS) `other`.  Counts only: no particular instruction is looked
for beyond the two load markers that name the loops.
"""
import argparse
import json
import os
import re
import sys

PRODUCTION = r"trace_simpleILb0ELb0ELi(33280|37376|41472)ELi2E"
CLASSES = ("valu", "salu", "branch", "wait", "vmem", "smem", "other")
_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_INSTR = re.compile(r"^\s*([a-z][a-z0-9_]*)\b(.*)$")


def classify(mnemonic):
    m = mnemonic
    if m.startswith("v_"):
        return "valu"
    if m.startswith("s_load") or m.startswith("s_buffer_load"):
        return "smem"
    if m.startswith("s_branch") or m.startswith("s_cbranch"):
        return "branch"
    if m.startswith("s_waitcnt") or m.startswith("s_nop") or m.startswith("s_sleep"):
        return "wait"
    if m.startswith("s_"):
        return "salu"
    if m.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    return "other"


class Block:
    def __init__(self, label):
        self.label = label          # None for a fall-through block
        self.ins = []               # (mnemonic, operands)
        self.succ = []              # block indices

    def counts(self):
        c = dict.fromkeys(CLASSES, 0)
        for m, _ in self.ins:
            c[classify(m)] += 1
        return c


def kernels(text):
    """{symbol: [Block]} for every function in the assembly text."""
    out = {}
    name, blocks = None, None
    for line in text.splitlines():
        code = line.split(";", 1)[0].rstrip()
        if not code.strip():
            continue
        lab = _LABEL.match(code)
        if lab:
            sym = lab.group(1)
            if sym.startswith(".L"):
                if blocks is not None:
                    blocks.append(Block(sym))
            else:
                name, blocks = sym, [Block(sym)]
                out[name] = blocks
            continue
        if blocks is None or code.lstrip().startswith("."):
            if code.strip().startswith(".end_amdhsa_kernel") or code.strip().startswith(".section"):
                name, blocks = None, None
            continue
        ins = _INSTR.match(code)
        if not ins:
            continue
        m, ops = ins.group(1), ins.group(2).strip()
        blocks[-1].ins.append((m, ops))
        if m.startswith("s_branch") or m.startswith("s_cbranch") or m in ("s_endpgm", "s_setpc_b64"):
            blocks.append(Block(None))
    for blocks in out.values():
        _link(blocks)
    return out


def _link(blocks):
    at = {b.label: i for i, b in enumerate(blocks) if b.label}
    for i, b in enumerate(blocks):
        last = b.ins[-1] if b.ins else None
        fall = True
        if last:
            m, ops = last
            if m.startswith("s_branch") or m.startswith("s_cbranch"):
                t = ops.split(",")[-1].strip()
                if t in at:
                    b.succ.append(at[t])
                fall = m.startswith("s_cbranch")
            elif m in ("s_endpgm", "s_setpc_b64"):
                fall = False
        if fall and i + 1 < len(blocks):
            b.succ.append(i + 1)


def _dominators(blocks):
    n = len(blocks)
    pred = [[] for _ in range(n)]
    for i, b in enumerate(blocks):
        for s in b.succ:
            pred[s].append(i)
    # reverse postorder from the entry
    order, seen, stack = [], [False] * n, [(0, 0)]
    seen[0] = True
    while stack:
        v, k = stack.pop()
        if k < len(blocks[v].succ):
            stack.append((v, k + 1))
            w = blocks[v].succ[k]
            if not seen[w]:
                seen[w] = True
                stack.append((w, 0))
        else:
            order.append(v)
    order.reverse()
    rank = {v: i for i, v in enumerate(order)}
    idom = {0: 0}

    def meet(a, b):
        while a != b:
            while rank[a] > rank[b]:
                a = idom[a]
            while rank[b] > rank[a]:
                b = idom[b]
        return a

    changed = True
    while changed:
        changed = False
        for v in order[1:]:
            new = None
            for p in pred[v]:
                if p in idom:
                    new = p if new is None else meet(p, new)
            if new is not None and idom.get(v) != new:
                idom[v] = new
                changed = True
    return idom, pred


def loops(blocks):
    """Natural loops, {header: set(blocks)}, back edges to one header merged."""
    idom, pred = _dominators(blocks)

    def dominates(h, v):
        while True:
            if v == h:
                return True
            if v not in idom or idom[v] == v:
                return False
            v = idom[v]

    out = {}
    for t, b in enumerate(blocks):
        if t not in idom:
            continue
        for h in b.succ:
            if dominates(h, t):
                body = out.setdefault(h, {h})
                work = [t]
                while work:
                    v = work.pop()
                    if v not in body:
                        body.add(v)
                        work.extend(p for p in pred[v] if p in idom)
    return out


def _marks(block, kind):
    if kind == "lockstep":
        return sum(1 for m, ops in block.ins if m == "buffer_load_dwordx4" and "offen" in ops)
    return sum(1 for m, _ in block.ins if m == "s_load_dwordx8")


def find_loop(blocks, all_loops, kind):
    """(header, body) of the innermost loop with the kind's loads, or None."""
    need = 2 if kind == "lockstep" else 1
    best = None
    for h, body in all_loops.items():
        if sum(_marks(blocks[v], kind) for v in body) >= need:
            if best is None or len(body) < len(best[1]):
                best = (h, body)
    return best


SKIP_VALU = 16      # a skippable region this long is the triangle test


def _region(blocks, body, header, start, join):
    """Blocks reached from `start` inside the loop before `join`, or None
    when `join` does not follow (the branch is no forward skip)."""
    seen, work, joined = set(), [start], start == join
    while work:
        v = work.pop()
        if v in seen or v == join:
            continue
        seen.add(v)
        for w in blocks[v].succ:
            if w == join:
                joined = True
            elif w in body and w != header:
                work.append(w)
    return seen if joined else None


def step_path(blocks, header, body, kind):
    """Blocks of the internal-node path, once round the loop from its header.
    At a conditional branch that skips a region forward, the region is skipped
    when it holds a load (a leaf's further loads) or SKIP_VALU or more vector
    instructions (the triangle test), unless the loop's loads of `kind` are
    all inside it (the step itself, under the lanes that walk); it is entered
    otherwise (bookkeeping that a step with lanes still walking runs).  At
    any other branch the path stays in the loop, on the side with fewer
    instructions ahead."""
    need = 2 if kind == "lockstep" else 1
    path, v = [], header
    while True:
        if v in path:
            return None                       # irreducible or an inner loop
        path.append(v)
        nxt = [w for w in blocks[v].succ if w in body]
        if not nxt:
            return None
        if len(nxt) == 1:
            w = nxt[0]
        else:
            taken, fall = nxt[0], nxt[1]
            region = _region(blocks, body, header, fall, taken)
            if region is not None:
                c = _sum(blocks, region)
                leaf = c["vmem"] + c["smem"] > 0 or c["valu"] >= SKIP_VALU
                rest = sum(_marks(blocks[x], kind) for x in body if x not in region)
                w = taken if leaf and rest >= need else fall
            elif header in nxt:
                w = header
            else:
                w = min(nxt, key=lambda x: len(blocks[x].ins))
        if w == header:
            return path
        v = w


def _sum(blocks, ids):
    c = dict.fromkeys(CLASSES, 0)
    for v in ids:
        for k, n in blocks[v].counts().items():
            c[k] += n
    return c


def count_kernel(blocks):
    """{kind: {"path": counts, "loop": counts, "scratch": n, "blocks": n}}."""
    res = {}
    all_loops = loops(blocks)
    for kind in ("lockstep", "solo"):
        found = find_loop(blocks, all_loops, kind)
        if not found:
            continue
        h, body = found
        path = step_path(blocks, h, body, kind)
        if path is None:
            continue
        res[kind] = {
            "path": _sum(blocks, path),
            "loop": _sum(blocks, sorted(body)),
            "scratch": sum(1 for v in body for m, _ in blocks[v].ins if m.startswith("scratch_")),
            "blocks": len(body),
            "path_blocks": [blocks[v].label or f"#{v}" for v in path],
        }
    return res


def count_text(text, pattern=PRODUCTION):
    rx = re.compile(pattern)
    return {name: count_kernel(blocks) for name, blocks in kernels(text).items() if rx.search(name)}


def render(result):
    lines = []
    head = f"{'kernel':<44} {'loop':<9}" + "".join(f"{c:>7}" for c in CLASSES) + f"{'scratch':>9}"
    lines.append(head)
    for name in sorted(result):
        short = re.search(r"trace_simpleI(\w+?)EEv", name)
        short = ("trace_simple<" + short.group(1) + ">") if short else name
        for kind, r in result[name].items():
            lines.append(f"{short[:44]:<44} {kind:<9}" + "".join(f"{r['path'][c]:>7}" for c in CLASSES) +
                         f"{r['scratch']:>9}")
            lines.append(f"{'':<44} {'(whole)':<9}" + "".join(f"{r['loop'][c]:>7}" for c in CLASSES))
    return "\n".join(lines)


def main(argv=None):
    here = os.path.dirname(os.path.abspath(__file__))
    default = os.path.join(here, "..", "3d-ray-tracer-vulkan_amd", "build", "rt_trace-hip-amdgcn-amd-amdhsa-gfx950.s")
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("asm", nargs="?", default=default)
    ap.add_argument("--kernel", default=PRODUCTION, help="regex over kernel symbols")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args(argv)
    with open(a.asm) as f:
        result = count_text(f.read(), a.kernel)
    if not result:
        print("no kernel matches", a.kernel, file=sys.stderr)
        return 1
    print(json.dumps(result, indent=1, sort_keys=True) if a.json else render(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
