"""Light rows of the band sweep (lgc_sweep_cfg.light_len) on small operators: the cases and what a plan must satisfy.

Shared by tests/test_sweep_light_host.py (host planner, no GPU) and tests/test_sweep_light_gpu.py (device planner and
kernels).  The operators are built with tests/sweep_support.py's ``_embed`` (a CSR slice inside a larger CSR); every one
has at most a few hundred rows and at most 4 k entries.  Columns are drawn so that the bands, which the planner cuts at
equal entry counts, come out where a case needs them.
"""
import numpy as np

import sweep_support as ss


def _mixed():
    """Rows of 0..39 entries and three long ones over 1200 columns: light and heavy rows side by side."""
    rng = np.random.default_rng(201)
    lens = rng.integers(0, 40, size=70)
    lens[[4, 20, 51]] = (260, 180, 90)
    lens[[9, 10]] = 0
    return ss._embed("light_mixed", 21, [rng.choice(1200, size=n, replace=False) for n in lens], 7, 1200, 1300)


def _threshold():
    """Rows of exactly 24 and exactly 25 entries next to each other (the threshold of the tests is 24)."""
    rng = np.random.default_rng(202)
    lens = [24, 25] * 12 + [23, 26, 24, 25]
    return ss._embed("light_threshold", 22, [rng.choice(800, size=n, replace=False) for n in lens], 0, 800, 3)


def _one_band_of_a_pair():
    """Two rows in three have six entries in the middle of ONE eighth of the columns (rows 3j and 3j + 1 in eighth j % 8,
    so every eighth gets as many and the eight bands stay close to the eighths): light rows whose pair has an empty
    run, for either row parity and on either side of the pair.  Every third row has 30 entries anywhere."""
    rng = np.random.default_rng(203)
    rows = []
    for i in range(48):
        if i % 3 == 2:
            rows.append(rng.choice(800, size=30, replace=False))
        else:
            rows.append(((i // 3) % 8) * 100 + 10 + rng.choice(80, size=6, replace=False))
    return ss._embed("light_one_band", 23, rows, 11, 800, 900)


def _empty_band():
    """Half of all entries sit in ONE column: with eight bands cut at equal entry counts several bands have no column
    at all (bound[b] == bound[b + 1])."""
    rng = np.random.default_rng(204)
    rows = [np.concatenate([np.zeros(10, dtype=np.int64), 1 + rng.choice(300, size=10, replace=False)]) for _ in range(40)]
    return ss._embed("light_empty_band", 24, rows, 5, 301, 400)


def _long_light_run():
    """Rows of 150 entries, all of them in two neighbouring bands: light under a threshold of 160, and the pair's run is
    long enough for the piece cap (16 in the tests, raised to at most 64) to cut it."""
    rng = np.random.default_rng(205)
    rows = [rng.choice(90, size=75, replace=False) for _ in range(8)]
    rows = [np.concatenate([r, 400 + rng.choice(90, size=75, replace=False)]) for r in rows]
    rows += [rng.choice(490, size=n, replace=False) for n in rng.integers(1, 30, size=10)]
    return ss._embed("light_long_run", 25, rows, 2, 490, 600)


def _rounds():
    """36 rows of 16 entries spread over all columns: with eight bands, four wavefronts per band and round and three
    accumulators each, 36 pieces per band are three rounds of twelve; as light rows they are 18 per band: two."""
    rng = np.random.default_rng(206)
    rows = [np.sort(np.concatenate([b * 100 + rng.choice(100, size=2, replace=False) for b in range(8)])) for _ in range(36)]
    return ss._embed("light_rounds", 26, rows, 3, 800, 850)


_BUILDERS = {"light_mixed": _mixed, "light_threshold": _threshold, "light_one_band": _one_band_of_a_pair,
             "light_empty_band": _empty_band, "light_long_run": _long_light_run, "light_rounds": _rounds}
OPERATORS = tuple(_BUILDERS)
_cases = {}


def case(name) -> ss.Case:
    if name not in _cases:
        _cases[name] = _BUILDERS[name]()
    return _cases[name]


def _cfg(**kw):
    return {**dict(n_bands=8, waves_per_band_round=4, row_cap=78, piece_cap=64, lookahead=64, groups=4, round_order=2,
                   light_len=24), **kw}


# (operator, configuration name, configuration).  light_len 24 unless a case says otherwise; 10 ** 6 = all rows light,
# 1 on rows of >= 2 entries = no row light.
PLANS = [
    ("light_mixed", "b8", _cfg()),
    ("light_mixed", "b2", _cfg(n_bands=2)),
    ("light_mixed", "b8_small", _cfg(row_cap=5, piece_cap=4, lookahead=4)),
    ("light_mixed", "b8_order0", _cfg(row_cap=7, piece_cap=8, round_order=0)),
    ("light_mixed", "b8_order1", _cfg(row_cap=7, piece_cap=8, round_order=1)),
    ("light_mixed", "b8_g2", _cfg(row_cap=51, groups=2)),
    ("light_mixed", "b8_all_light", _cfg(light_len=10 ** 6, row_cap=9)),
    ("light_threshold", "b8", _cfg()),
    ("light_threshold", "b2", _cfg(n_bands=2, row_cap=6)),
    ("light_threshold", "b8_none_light", _cfg(light_len=1)),
    ("light_one_band", "b8", _cfg(row_cap=11)),
    ("light_one_band", "b2", _cfg(n_bands=2)),
    ("light_empty_band", "b8", _cfg(row_cap=4)),
    ("light_long_run", "b8_pcap16", _cfg(light_len=160, piece_cap=16, row_cap=6)),
    ("light_rounds", "b8_cap3", _cfg(row_cap=3)),
]
PLAN_IDS = [f"{o}-{n}" for o, n, _ in PLANS]


def row_lengths(c: ss.Case):
    rp = c.rowptr.numpy()
    return rp[c.row_begin + 1:c.row_end + 1] - rp[c.row_begin:c.row_end]


def band_bounds(c: ss.Case, n_bands):
    """The planner's bands: column ranges with (nearly) equal entry counts (phase A)."""
    cols = c.entries.numpy()[c.rowptr[c.row_begin]:c.rowptr[c.row_end], 0]
    hist = np.bincount(cols - c.col_lo, minlength=c.col_hi - c.col_lo)
    ne, run, b = int(hist.sum()), 0, 1
    bound = [c.col_hi] * (n_bands + 1)
    bound[0] = c.col_lo
    for col, h in enumerate(hist):
        if b >= n_bands:
            break
        run += int(h)
        while b < n_bands and run * n_bands >= ne * b and ne > 0:
            bound[b] = c.col_lo + col + 1
            b += 1
    return bound


def band_of(col, bound):
    b = 0
    while b + 1 < len(bound) - 1 and col >= bound[b + 1]:
        b += 1
    return b


def check_light_plan(c: ss.Case, cfg, dims, arr):
    """Everything the issue asks of a plan with light rows.  Returns {slot: [(col, value bits)]} of the decoded plan."""
    row_cap, nb, light = cfg["row_cap"], cfg["n_bands"], cfg["light_len"]
    assert dims["light_len"] == light and dims["n_bands"] == nb
    got = ss.decode_sweep(dims, arr, row_cap)                 # no step holds two entries of one piece; padding well-formed
    wnp = arr["wave_npieces"].numpy()[: dims["n_waves"]]
    assert (wnp <= row_cap).all() and wnp.sum() == dims["n_slots"]
    assert dims["n_waves"] == dims["rounds"] * cfg["waves_per_band_round"] * nb
    multi = arr["multi"].numpy()
    n_rows = c.row_end - c.row_begin
    assert multi.shape == (n_rows, 4) and (multi[:, 0] == np.arange(c.row_begin, c.row_end)).all()
    assert multi[0, 1] == 0 and multi[-1, 2] == dims["n_slots"] and (multi[1:, 1] == multi[:-1, 2]).all()
    assert sorted(got) == list(range(dims["n_slots"]))
    # slot -> the band of the wavefront that holds it
    ps = arr["piece_slot"].numpy().reshape(-1, row_cap)
    home = {}
    for w in range(dims["n_waves"]):
        for lp in range(wnp[w]):
            assert int(ps[w, lp]) not in home
            home[int(ps[w, lp])] = (w // 4) % nb
    bound = band_bounds(c, nb)
    lens = row_lengths(c)
    for i, (row, sb, se, _) in enumerate(multi):
        ent = c.entries[c.rowptr[row]:c.rowptr[row + 1]]
        want = sorted((int(col), int(v) & 0xFFFFFFFF) for col, v in ent.tolist())
        mine = [e for sl in range(sb, se) for e in got[sl]]
        assert sorted(mine) == want, row                      # every entry exactly once, in a slot of its own row
        assert all(len(got[sl]) <= dims["piece_cap"] for sl in range(sb, se))
        homes = [home[sl] for sl in range(sb, se)]
        is_light = lens[i] <= light
        for sl in range(sb, se):
            bands = {band_of(col, bound) for col, _ in got[sl]}
            if is_light:                                      # one pair of bands per piece, at home in one of the two
                assert len({b // 2 for b in bands}) == 1 and home[sl] // 2 == next(iter(bands)) // 2, (row, sl)
                other = home[sl] ^ 1
                run = {b: sum(band_of(int(col), bound) == b for col, _ in want) for b in (home[sl], other)}
                if run[home[sl]] and run[other]:
                    assert home[sl] == (home[sl] & ~1) + (i & 1), (row, sl)
                else:
                    assert run[home[sl]] > 0, (row, sl)      # an empty run: the piece lives where the entries are
            else:
                assert bands == {home[sl]}, (row, sl)
        assert [h // 2 for h in homes] == sorted(h // 2 for h in homes), row       # band-major slots
    return got
