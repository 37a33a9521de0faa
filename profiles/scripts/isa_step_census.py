#!/usr/bin/env python3
"""Instruction census of one kernel, per basic block and by class, and of the loop that holds its f64 divisions.

usage: isa_step_census.py file.s kernel_regex [--divs R] [--unroll K] [--blocks]

file.s is `hipcc --cuda-device-only -S` output.  The kernel is the first function label that matches kernel_regex.  A basic
block is the run of instructions between two `.LBBn_m:` labels.  Classes:
  f64     v_add_f64 / v_mul_f64 / v_fma_f64 (also the fmas of a division's Newton steps: the ISA does not tell them apart)
  div     v_div_scale_f64 / v_rcp_f64 / v_div_fmas_f64 / v_div_fixup_f64
  sel     v_cndmask_* / v_cmp_* / v_cmpx_*
  salu    every s_* instruction that is not a wait or a branch
  branch  s_branch / s_cbranch_* / s_setpc / s_swappc
  lds     ds_*
  gld     global_load_* / scratch_load_*        gst   global_store_* / scratch_store_*
  wait    s_waitcnt* / s_nop / s_sleep
  valu    every other v_* instruction
A basic block ends at a label or behind a branch.  The "division loop" is ONE trip round the loop that holds the f64 divisions: the
closed path through the control-flow graph that issues a given number of v_rcp_f64 with the fewest instructions, i.e. the path that
skips every fallback block behind a wave-uniform branch.  (A natural loop -- every block that reaches a backward branch -- is no use
here: when several code paths share a loop, as the four integrators do in one kernel, it is their union.)  Without --divs the trip
is the one with the most divisions among the cheapest trips that pass no block twice (cart-pole RK4, two steps per trip of the
ping-pong loop: 16); --divs R asks for a trip of R divisions -- needed where one loop holds several integrators behind run-time
tests (the kernel before round 10): a static path may then mix them, and only the division count names the trip that runs.  Printed: the instruction total of the cheapest trip for every division
count that has one, then the census of every block of the chosen trip, their sum, and with --unroll K the sum divided by K (steps per
trip).  --blocks prints every block of the kernel first."""
import re
import sys

CLASSES = ["f64", "div", "sel", "salu", "branch", "lds", "gld", "gst", "wait", "valu"]


def classify(op):
    if op in ("v_add_f64", "v_mul_f64", "v_fma_f64") or op.startswith(("v_add_f64_", "v_mul_f64_", "v_fma_f64_")):
        return "f64"
    if op.startswith(("v_div_scale_f64", "v_rcp_f64", "v_div_fmas_f64", "v_div_fixup_f64")):
        return "div"
    if op.startswith(("v_cndmask", "v_cmp")):
        return "sel"
    if op.startswith(("s_waitcnt", "s_nop", "s_sleep")):
        return "wait"
    if op.startswith(("s_branch", "s_cbranch", "s_setpc", "s_swappc")):
        return "branch"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_load", "scratch_load", "flat_load", "buffer_load")):
        return "gld"
    if op.startswith(("global_store", "scratch_store", "flat_store", "buffer_store", "global_atomic")):
        return "gst"
    if op.startswith("v_"):
        return "valu"
    return "salu"


def is_branch(op):
    return op.startswith(("s_branch", "s_cbranch"))


def kernel_blocks(path, rx):
    """[(label, [(op, text), ...]), ...] of the first function whose label matches rx; a block ends at a label or behind a branch"""
    lines = open(path).read().split("\n")
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l) and re.search(rx, l)]
    if not starts:
        sys.exit("no kernel matches %r" % rx)
    start = starts[0]
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    blocks = [("entry", [])]
    for l in lines[start + 1:end]:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            blocks.append((m.group(1), []))
            continue
        t = l.strip()
        if not l.startswith("\t") or not t or t.startswith((".", ";")):
            continue
        if blocks[-1][1] and is_branch(blocks[-1][1][-1][0]):
            blocks.append((blocks[-1][0].split("+")[0] + "+%d" % len(blocks), []))
        blocks[-1][1].append((t.split()[0], t))
    return lines[start].rstrip(":"), blocks


def successors(blocks):
    index = {lab: i for i, (lab, _) in enumerate(blocks)}
    succ = []
    for j, (_, insts) in enumerate(blocks):
        s, fall = set(), True
        if insts:
            op, text = insts[-1]
            if is_branch(op):
                tgt = text.split()[-1]
                if tgt in index:
                    s.add(index[tgt])
                fall = op != "s_branch"
            elif op == "s_endpgm" or op.startswith("s_setpc"):
                fall = False
        if fall and j + 1 < len(blocks):
            s.add(j + 1)
        succ.append(s)
    return succ


def n_rcp(insts):
    return sum(op.startswith("v_rcp_f64") for op, _ in insts)


def natural_loops(blocks, succ):   # (kept for interactive use; main() does not rely on it)
    """{header: set of blocks} over every backward branch (loops that share a header are merged)"""
    pred = [set() for _ in blocks]
    for j, s in enumerate(succ):
        for k in s:
            pred[k].add(j)
    loops = {}
    for j, s in enumerate(succ):
        for h in s:
            if h <= j:
                body, todo = {h}, [j]
                while todo:
                    n = todo.pop()
                    if n not in body:
                        body.add(n)
                        todo.extend(pred[n])
                loops.setdefault(h, set()).update(body)
    return loops


def cheapest_trips(blocks, succ, cap):
    """{R: (instructions, [blocks])}: for every division count R <= cap, the closed path with exactly R v_rcp_f64 and the fewest instructions"""
    import heapq
    rc = [n_rcp(insts) for _, insts in blocks]
    best = {}
    for h in sorted({k for j, s in enumerate(succ) for k in s if k <= j}):
        if rc[h] > cap:
            continue
        dist = {(h, rc[h]): len(blocks[h][1])}
        back = {}
        heap = [(len(blocks[h][1]), h, rc[h])]
        while heap:
            dcur, n, r = heapq.heappop(heap)
            if dist.get((n, r), 1 << 60) < dcur:
                continue
            for k in succ[n]:
                if k == h:
                    if r > 0 and (r not in best or dcur < best[r][0]):
                        path, key = [], (n, r)
                        while key in back:
                            path.append(key[0]); key = back[key]
                        path.append(h)
                        best[r] = (dcur, path[::-1])
                    continue
                r2 = r + rc[k]
                d2 = dcur + len(blocks[k][1])
                if r2 <= cap and d2 < dist.get((k, r2), 1 << 60):
                    dist[(k, r2)] = d2; back[(k, r2)] = (n, r)
                    heapq.heappush(heap, (d2, k, r2))
    return best


def count(insts):
    c = dict.fromkeys(CLASSES, 0)
    for op, _ in insts:
        c[classify(op)] += 1
    return c


def row(name, c, div=1):
    tot = sum(c.values())
    f = (lambda v: "%6d" % v) if div == 1 else (lambda v: "%6.1f" % (v / div))
    return "%-12s %s  %s" % (name, " ".join(f(c[k]) for k in CLASSES), f(tot))


def main():
    argv = sys.argv[1:]
    opt = {}
    for key in ("--unroll", "--divs"):
        if key in argv:
            k = argv.index(key)
            opt[key] = int(argv[k + 1])
            del argv[k:k + 2]
    args = [a for a in argv if not a.startswith("--")]
    unroll = opt.get("--unroll", 1)
    name, blocks = kernel_blocks(args[0], args[1])
    succ = successors(blocks)
    print(name)
    print("%-12s %s  %6s" % ("block", " ".join("%6s" % k for k in CLASSES), "total"))
    if "--blocks" in argv:
        for lab, insts in blocks:
            print(row(lab, count(insts)))
        print(row("kernel", count([i for _, insts in blocks for i in insts])))
    total_rcp = n_rcp([i for _, insts in blocks for i in insts])
    trips = cheapest_trips(blocks, succ, opt.get("--divs", min(total_rcp, 64)))
    if "--divs" in opt:
        divs = opt["--divs"]
        if divs not in trips:
            print("no closed path with %d v_rcp_f64" % divs)
            return
    else:   # the trip with the most divisions that passes no block twice
        simple = [r for r, (_, path) in trips.items() if len(set(path)) == len(path)]
        if not simple:
            print("no loop with a v_rcp_f64")
            return
        divs = max(simple)
    path = trips[divs][1]
    print("closed paths, v_rcp_f64: instructions -- " + ", ".join("%d: %d" % (r, trips[r][0]) for r in sorted(trips)))
    print("division loop: cheapest trip with %d v_rcp_f64, %d blocks from %s" % (divs, len(path), blocks[path[0]][0]))
    body = [i for b in path for i in blocks[b][1]]
    for b in path:
        print(row(blocks[b][0], count(blocks[b][1])))
    print(row("loop", count(body)))
    if unroll > 1:
        print(row("per step", count(body), unroll))


if __name__ == "__main__":
    main()
