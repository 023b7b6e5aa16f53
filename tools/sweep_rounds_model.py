#!/usr/bin/env python3
"""What light rows (lgc_sweep_cfg.light_len) do to the band-sweep plan of the item half, counted on the CPU.

    python tools/sweep_rounds_model.py [--config cosmetics|small] [--light 0 100 120 140 160 200] [--pcap 0]

A numpy restatement of the planner's phases A-C (csrc/lgconv_hip.hip, plan_pieces_and_deal): bands by equal entry
counts, one piece per (row, band) -- per (row, pair of bands) for a light row, at home in band 2k + (row & 1) or where
the entries are -- cut at the piece cap (the configured 64 raised in steps of 16 while that saves a round, or --pcap N
fixed), rounds filled by piece weight.  For the full item half, the reduced one (users of degree <= T eliminated,
DESIGN section 17), the reduced one concatenated with G_L (same section) and every threshold it prints

    light rows, their share of the entries, pieces, the most-loaded band, rounds, the partial rows' bytes (256 B per
    piece at D = 64) and the compulsory row fetches: distinct (executing band, round, user row) triples, i.e. how often
    a gathered row must cross the fabric if nothing drifts (DESIGN section 5 measures ~2.3 per used row where this
    model says 2.15).

No GPU and no library: the numbers for the next change of the planner.  The planner's own figures (pieces, rounds,
cap) come back in lgc_sweep_dims and must agree with this table.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_ecommerce_amd import synth  # noqa: E402

NB, WPBR, CAP, PIECE_CAP = 8, 256, 78, 64


def item_half(user, item, n_users, max_deg):
    """(row of every entry, column of every entry), sorted by (row, column); users of degree <= max_deg dropped and the
    rest renumbered, as build_reduced_csr does."""
    if max_deg > 0:
        keep = np.bincount(user, minlength=n_users) > max_deg
        sel = keep[user]
        user, item = np.cumsum(keep)[user[sel]] - 1, item[sel]
    order = np.lexsort((user, item))
    return item[order].astype(np.int64), user[order].astype(np.int64)


def concat_half(user, item, n_users, n_items, max_deg):
    """(row, column, columns) of the concatenated operator [R_H^T | G_L] (lgc_reduce_concat): the kept
    users renumbered around NB gaps of ceil(n_items / NB) rows, gap b where band b's share of R_H^T's entries ends, and the
    pattern of G_L = R_L^T R_L with column j at item j's row inside its gap."""
    deg = np.bincount(user, minlength=n_users)
    row, col = item_half(user, item, n_users, max_deg)
    n_h = int(col.max()) + 1
    bound = bands(col, n_h)
    gap_rows = -(-n_items // NB)
    phys = col + gap_rows * np.searchsorted(bound[1:NB], col, side="right")
    gap_start = bound[1:NB + 1] + gap_rows * np.arange(NB)
    sel = (deg <= max_deg)[user]
    u, it = user[sel], item[sel]
    order = np.argsort(u, kind="stable")
    u, it = u[order], it[order]
    start = np.concatenate(([0], np.cumsum(np.bincount(u, minlength=n_users))))[u]
    pi, pj = [], []
    for k in range(max_deg):                     # entry (u, i) times the k-th entry of u's row
        ok = deg[u] > k
        pi.append(it[ok])
        pj.append(it[start[ok] + k])
    key = np.unique(np.concatenate(pi).astype(np.int64) * n_items + np.concatenate(pj))
    gi, gj = key // n_items, key % n_items
    row, col = np.concatenate((row, gi)), np.concatenate((phys, gap_start[gj // gap_rows] + gj % gap_rows))
    order = np.lexsort((col, row))
    return row[order], col[order], n_h + NB * gap_rows


def bands(col, n_cols):
    cum = np.cumsum(np.bincount(col, minlength=n_cols))
    ne = int(cum[-1])
    bound = np.full(NB + 1, n_cols, dtype=np.int64)
    bound[0] = 0
    for b in range(1, NB):                       # first column c with cum[c] * NB >= ne * b -> bound c + 1
        bound[b] = min(int(np.searchsorted(cum * NB, ne * b, side="left")) + 1, n_cols)
    return bound


def runs(run_len, light):
    """(row, home band, count, first band) of every run that becomes pieces, in slot order."""
    n_rows = run_len.shape[0]
    is_light = (run_len.sum(1) <= light) if light > 0 else np.zeros(n_rows, dtype=bool)
    rows = np.arange(n_rows)
    h_rows, l_rows = rows[~is_light], rows[is_light]
    heavy = (np.repeat(h_rows, NB), np.tile(np.arange(NB), h_rows.size), run_len[h_rows].ravel())
    lo, hi = run_len[l_rows][:, 0::2], run_len[l_rows][:, 1::2]
    pair = np.tile(np.arange(0, NB, 2), l_rows.size).reshape(l_rows.size, NB // 2)
    home = np.where(lo == 0, pair + 1, np.where(hi == 0, pair, pair + (l_rows & 1)[:, None]))
    lightp = (np.repeat(l_rows, NB // 2), home.ravel(), (lo + hi).ravel())
    row, band, cnt = (np.concatenate(x) for x in zip(heavy, lightp))
    order = np.lexsort((band, row))              # slots: row-major, then by band (a pair's piece sits at its home band)
    row, band, cnt = row[order], band[order], cnt[order]
    live = cnt > 0
    return row[live], band[live], cnt[live], int(is_light.sum()), int(run_len[is_light].sum())


def most_loaded(band, cnt, pcap):
    return int(np.bincount(band, weights=-(-cnt // pcap), minlength=NB).max())


def plan(run_len, light, fixed_pcap):
    row, band, cnt, n_light, e_light = runs(run_len, light)
    rounds_for = lambda p: max(1, -(-most_loaded(band, cnt, p) // (WPBR * CAP)))
    pcap = fixed_pcap or PIECE_CAP
    if not fixed_pcap:
        fewest = rounds_for(1 << 40)
        while pcap < 4 * PIECE_CAP and rounds_for(pcap) > fewest:
            pcap += 16
    rounds = rounds_for(pcap)
    parts = -(-cnt // pcap)
    per = -(-cnt // parts)
    n_p = -(-cnt // per)
    p_run = np.repeat(np.arange(cnt.size), n_p)
    p_idx = np.arange(p_run.size) - np.repeat(np.cumsum(n_p) - n_p, n_p)
    p_cnt = np.minimum(per[p_run], cnt[p_run] - p_idx * per[p_run])
    p_band = band[p_run]
    # rounds by weight: inside a band the heaviest ceil(n / rounds) pieces are round 0, the next round 1, ...
    p_round = np.zeros(p_run.size, dtype=np.int64)
    for b in range(NB):
        idx = np.flatnonzero(p_band == b)
        idx = idx[np.argsort(-p_cnt[idx], kind="stable")]
        p_round[idx] = np.arange(idx.size) // max(1, -(-idx.size // rounds))
    return dict(light_rows=n_light, light_entries=e_light, pieces=int(p_run.size), most=most_loaded(band, cnt, pcap),
                rounds=rounds, pcap=pcap, p_cnt=p_cnt, p_band=p_band, p_round=p_round)


def fetches(col, p, n_cols):
    """Distinct (band, round, column): the pieces cover the (row, column)-sorted entries in order."""
    key = np.repeat(p["p_band"] * p["rounds"] + p["p_round"], p["p_cnt"])
    return int(np.unique(key * n_cols + col).size)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", choices=["cosmetics", "small"], default="cosmetics")
    ap.add_argument("--light", type=int, nargs="*", default=[0, 100, 120, 140, 160, 200])
    ap.add_argument("--pcap", type=int, default=0, help="a fixed piece cap (0: the planner's rule)")
    ap.add_argument("--max-deg", type=int, default=3, help="T of the reduced item half")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    cfg = synth.CONFIG_COSMETICS if args.config == "cosmetics" else synth.CONFIG_SMALL
    g = synth.make_bipartite(**cfg, seed=args.seed)
    print("| operator | light_len | light rows | their entries | pieces | most in a band | piece cap | rounds | partial rows "
          "| row fetches | per used row |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for name, max_deg in (("concatenated [R_H^T | G_L] (T=%d)" % args.max_deg, -args.max_deg),
                          ("reduced item half (T=%d)" % args.max_deg, args.max_deg), ("full item half", 0)):
        if max_deg < 0:
            row, col, n_cols = concat_half(g.user, g.item, g.n_users, g.n_items, -max_deg)
        else:
            row, col = item_half(g.user, g.item, g.n_users, max_deg)
            n_cols = int(col.max()) + 1
        bound = bands(col, n_cols)
        band = np.searchsorted(bound[1:NB], col, side="right")
        run_len = np.bincount(row * NB + band, minlength=g.n_items * NB).reshape(g.n_items, NB)
        used = int(np.unique(col).size)
        for light in args.light:
            p = plan(run_len, light, args.pcap)
            f = fetches(col, p, n_cols)
            print(f"| {name} | {light} | {p['light_rows']:,} | {100.0 * p['light_entries'] / row.size:.1f} % | {p['pieces']:,} | "
                  f"{p['most']:,} | {p['pcap']} | {p['rounds']} | {p['pieces'] * 256 / 1e6:.0f} MB | "
                  f"{f / 1e6:.2f} M = {f * 256 / 1e9:.2f} GB | {f / used:.2f} |", flush=True)


if __name__ == "__main__":
    main()
