#!/usr/bin/env python3
"""What a query-order rebuild costs: from the rocpd .db of one traced fit (rocprofv3 --kernel-trace), the summed duration and
launch count of every rebuild (the kernels between two search launches that are not the launch-order sort) and the search launch
right after each rebuild -- which runs in plain launch order, every kept list gone -- next to the mean of its neighbours (the 4
launches before the rebuild and launches 3 .. 8 after it).   tools/rebuild_penalty.py <db>"""
import sqlite3
import sys

REBUILD = ("nn_qs_", "nn_order_keys_kernel", "sc_rs_hist_kernel", "sc_scan_kernel", "sc_rs_scatter_kernel")


def main(db):
    c = sqlite3.connect(db)
    rows = [(n, (e - s) / 1e3) for n, s, e in c.execute("select name, start, end from kernels order by start")]
    first = next(i for i, (n, _) in enumerate(rows) if "nn_stream4_kernel" in n)        # (the scene build's sort comes before it)
    search, rebuilds = [], []                     # durations of the search launches; (index of the search launch before it, us, launches)
    for n, d in rows[first:]:
        if "nn_stream4_kernel" in n:
            search.append(d)
        elif any(k in n for k in REBUILD):
            if rebuilds and rebuilds[-1][0] == len(search) - 1:
                rebuilds[-1][1] += d
                rebuilds[-1][2] += 1
            else:
                rebuilds.append([len(search) - 1, d, 1])
    print(f"{len(search)} search launches, mean {sum(search) / len(search):.2f} us; {len(rebuilds)} rebuilds, "
          f"mean {sum(r[1] for r in rebuilds) / max(len(rebuilds), 1):.1f} us in {sum(r[2] for r in rebuilds) / max(len(rebuilds), 1):.1f} launches")
    print("after launch | rebuild us (launches) | next search us | neighbours' mean us | penalty us")
    pen = []
    for at, us, k in rebuilds:
        nxt = search[at + 1] if at + 1 < len(search) else None
        nb = search[max(at - 3, 0):at + 1] + search[at + 3:at + 9]
        if nxt is None or not nb:
            print(f"{at:12d} | {us:8.1f} ({k}) | (the fit ends)")
            continue
        m = sum(nb) / len(nb)
        pen.append(nxt - m)
        print(f"{at:12d} | {us:8.1f} ({k}) | {nxt:8.1f} | {m:8.1f} | {nxt - m:+7.1f}")
    if pen:
        print(f"mean penalty of the launch after a rebuild: {sum(pen) / len(pen):+.1f} us over {len(pen)} rebuilds ({sum(pen):.0f} us per fit)")


if __name__ == "__main__":
    main(sys.argv[1])
