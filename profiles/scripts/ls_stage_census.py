#!/usr/bin/env python3
"""Census of the line-search ladder's launch shapes in a rocprofv3 --kernel-trace rocpd database of the headline command
(profiles/r13_inkernel_stages.md): rollout launches by grid height (whole ladder / stage 1 / stage 2), empty and non-empty
second stages, k_update by its place in the chain, k_costate_flush inside the iterations and at the end of a solve.
usage: ls_stage_census.py results.db [out.md] [n_alphas]"""
import sqlite3
import sys


def stat(v):
    if not v:
        return "0 launches"
    v = sorted(v)
    return "%d launches, average %.1f us, median %.1f, min %.1f, max %.1f" % (len(v), sum(v) / len(v) / 1e3, v[len(v) // 2] / 1e3, v[0] / 1e3, v[-1] / 1e3)


def main():
    c = sqlite3.connect(sys.argv[1])
    na = int(sys.argv[3]) if len(sys.argv) > 3 else 11
    t = [r[0] for r in c.execute("select name from sqlite_master where type in ('table', 'view')")]
    kd = [x for x in t if "kernel_dispatch" in x][0]
    ks = [x for x in t if "kernel_symbol" in x][0]
    scol = [r[1] for r in c.execute("pragma table_info(%s)" % ks)]
    namecol = "display_name" if "display_name" in scol else ("kernel_name" if "kernel_name" in scol else scol[-1])
    dcol = [r[1] for r in c.execute("pragma table_info(%s)" % kd)]
    qcol = "queue_id" if "queue_id" in dcol else ("stream_id" if "stream_id" in dcol else None)
    gy = [x for x in dcol if "grid" in x and x.endswith("y")]
    wy = [x for x in dcol if "workgroup" in x and x.endswith("y")]
    lines = ["dispatch columns: %s" % ", ".join(dcol), ""]
    if not gy:
        print("\n".join(lines)); print("no grid-height column: census not possible"); return
    rows = c.execute("select s.%s, d.start, d.end, %s, d.%s, %s from %s d join %s s on d.kernel_id = s.id order by d.start" %
                     (namecol, ("d." + qcol) if qcol else "0", gy[0], ("d." + wy[0]) if wy else "1", kd, ks)).fetchall()
    rows = [(n.replace("cddp_dev::", "").replace("void ", "").split("<")[0], a, b, q, int(g) // max(1, int(w))) for n, a, b, q, g, w in rows]
    queues = sorted({r[3] for r in rows})
    whole, st1, st2, upd = [], [], [], {"one-stage": [], "stage 1": [], "stage 2": []}
    flush_in, flush_end, sweeps, solves = [], [], [], 0
    for q in queues:
        seq = [r for r in rows if r[3] == q]
        # rollout launches of this queue: a launch below the whole ladder opens a two-stage pair, the next one closes it
        pend = None
        for n, a, b, _, h in seq:
            if not n.startswith("k_forward"): continue
            if pend is None and h >= na: whole.append(b - a)
            elif pend is None: pend = (b - a, h)
            else:
                st1.append(pend[0]); st2.append(b - a); pend = None
        # update / flush chain of this queue
        uf = [(n, b - a) for n, a, b, _, _ in seq if n.startswith(("k_update", "k_costate_flush", "k_value_merge"))]
        for i, (n, dt) in enumerate(uf):
            nxt = uf[i + 1][0] if i + 1 < len(uf) else ""
            prv = uf[i - 1][0] if i > 0 else ""
            if n.startswith("k_costate_flush"):
                (flush_end if nxt.startswith("k_value_merge") else flush_in).append(dt)
            elif n.startswith("k_update"):
                nn = uf[i + 2][0] if i + 2 < len(uf) else ""
                if nxt.startswith("k_costate_flush") and not nn.startswith("k_value_merge"): upd["stage 1"].append(dt)
                elif prv.startswith("k_costate_flush"): upd["stage 2"].append(dt)
                else: upd["one-stage"].append(dt)
        sweeps += [b - a for n, a, b, _, _ in seq if n.startswith("k_backward")]
        solves += sum(1 for n, _, _, _, _ in seq if n.startswith("k_init"))
    solves = max(1, solves)
    empty = [x for x in st2 if x < 10e3]
    full = [x for x in st2 if x >= 10e3]
    lines += ["group-solves (k_init launches): %d, ladder of %d step sizes" % (solves, na), "",
              "| item | figures | per group-solve |", "|---|---|---|",
              "| sweeps | %s | %.1f |" % (stat(sweeps), len(sweeps) / solves),
              "| rollout, whole ladder in one launch | %s | %.1f |" % (stat(whole), len(whole) / solves),
              "| rollout, stage 1 of a two-launch iteration | %s | %.1f |" % (stat(st1), len(st1) / solves),
              "| rollout, stage 2, empty (< 10 us) | %s | %.1f |" % (stat(empty), len(empty) / solves),
              "| rollout, stage 2, not empty | %s | %.1f |" % (stat(full), len(full) / solves)]
    for k in ("one-stage", "stage 1", "stage 2"):
        lines.append("| `k_update`, %s | %s | %.1f |" % (k, stat(upd[k]), len(upd[k]) / solves))
    lines += ["| `k_costate_flush` inside the iterations | %s | %.1f |" % (stat(flush_in), len(flush_in) / solves),
              "| `k_costate_flush` at the end of a solve | %s | %.1f |" % (stat(flush_end), len(flush_end) / solves)]
    out = "\n".join(lines)
    print(out)
    if len(sys.argv) > 2 and sys.argv[2] != "-":
        open(sys.argv[2], "w").write(out + "\n")


if __name__ == "__main__":
    main()
