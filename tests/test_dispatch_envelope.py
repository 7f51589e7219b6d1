"""The dispatcher of models/hipconv.py at the edges of what its rules admit — host logic and workspace probes only, no kernel is launched.

The rules were measured on square maps at batch 8 / 16, and several bound H alone, or H * W alone, and channel counts from below only: they
hand the engines elongated maps, one-row and one-column maps and other batches.  Three checks:
  * no answer of `select` / `select_wrw` over a grid with H != W is one the chosen engine's own support query refuses (such a layer would
    raise NotImplementedError in `conv_nobias` although torch computes it);
  * every row of tests/dispatch_envelope.py's corner table still reaches the engines it names (tests/test_gpu_dispatch_envelope.py runs
    those rows against fp64: a row whose answer moved to MIOpen would compare MIOpen with fp64 and pass);
  * the table covers every (engine, pass kind) the grid observes, in both orientations and at batches 1 and 3.
"""
import pytest

import dispatch_envelope as de

# H and W each: the rules' thresholds (4, 16, 32, 64, 128, 256), their neighbours, odd extents, one-row / one-column maps and 4096
EXTENTS = [1, 2, 3, 4, 5, 8, 16, 17, 31, 32, 34, 64, 66, 128, 130, 256, 4096]
BATCHES = [1, 3, 8, 16]
# the four geometries of the nets, and four the rules must tell from them: another pad of the dilated and of the one-channel layer, stride 2 at k3
GEOMS = [de.K3, de.S2, de.DIL, de.K4S1, (4, 2, 1, 2), (3, 1, 0, 1), (4, 1, 0, 1), (3, 2, 1, 1)]
# (Cin, Cout), thinned to the rules' channel thresholds and one count on either side of each: 1 / 3 / 6 on a side, 64, 128, 256, 512, a
# reduction that is no multiple of 16, a produced count that is no tile multiple
CHANNELS = [(3, 3), (3, 64), (64, 3), (64, 64), (128, 128), (128, 130), (256, 256), (512, 512)]
CHANNELS_DEFAULT = CHANNELS + [(6, 64), (128, 6), (64, 1), (80, 64), (256, 64)]
# name -> (environment switches, in-process switches (de.switches), the activation dtypes whose answers the setting can move, the channel pairs:
# the default switches get the longer list)
SETTINGS = [("default", {}, "default", (False, True), CHANNELS_DEFAULT),
            ("direct_bf16x3", {}, "direct_bf16x3", (False,), CHANNELS), ("direct_bf16x3_dw", {}, "direct_bf16x3_dw", (False,), CHANNELS),
            ("direct_bf16x3_s2", {}, "direct_bf16x3_s2", (False,), CHANNELS), ("direct_bf16x3_s2_dw", {}, "direct_bf16x3_s2_dw", (False,), CHANNELS),
            ("bf16_all", {"IPSR_BF16_ENGINES": "all"}, "default", (True,), CHANNELS_DEFAULT),
            ("engine_direct", {"IPSR_CONV_ENGINE": "direct"}, "default", (False, True), CHANNELS),
            ("engine_winograd", {"IPSR_CONV_ENGINE": "winograd"}, "default", (False, True), CHANNELS)]
_ENV_SWITCHES = ("IPSR_CONV_ENGINE", "IPSR_NO_SMALLMAP", "IPSR_NO_THIN", "IPSR_SMALLMAP_MAX_POS", "IPSR_BF16_ENGINES")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from deepinpainting_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def sweep(built):
    """-> (refused, seen): the answers the chosen engine's own support query refuses, as (setting, engine, kind, op, lay, bf16), and the
    {(engine, kind): count} of every answer other than "miopen", over settings x dtypes x batches x geometries x channels x H x W x the three
    passes of Conv2d and of ConvTranspose2d, on the shapes torch accepts."""
    from deepinpainting_amd import ops
    from deepinpainting_amd.models import hipconv
    assert sorted(n for n, _, sw, _, _ in SETTINGS if sw != "default") == sorted(ops.DIRECT_PASSES)
    mp = pytest.MonkeyPatch()
    refused, seen, points = [], {}, 0
    try:
        mp.setattr(hipconv, "_FORCE", None)
        for name, env, sw, dtypes, channels in SETTINGS:
            for var in _ENV_SWITCHES:
                mp.delenv(var, raising=False)
            for var, val in env.items():
                mp.setenv(var, val)
            hipconv.reload_env()
            with de.switches(hipconv, sw):
                for bf16 in dtypes:
                    for B in BATCHES:
                        for geom in GEOMS:
                            for Cin, Cout in channels:
                                for H in EXTENTS:
                                    for W in EXTENTS:
                                        for transposed in (False, True):
                                            lay = (transposed, B, Cin, H, W, Cout) + geom
                                            if not de.torch_accepts(lay):
                                                continue
                                            for eng, (kind, op) in zip(de.answers(hipconv, lay, bf16), de.passes(lay)):
                                                points += 1
                                                if eng == "miopen":
                                                    continue
                                                seen[(eng, kind)] = seen.get((eng, kind), 0) + 1
                                                if not de.takes(eng, kind, op, lay, bf16):
                                                    refused.append((name, eng, kind, op, lay, bf16))
                    hipconv._SEL.clear()             # the memo of a finished dtype is dead weight
    finally:
        mp.undo()
        hipconv.reload_env()
    print("dispatcher sweep: %d answers, %d on a HIP engine, %d refused" % (points, sum(seen.values()), len(refused)))
    return refused, seen


def test_no_selection_is_refused_by_its_engine(sweep):
    """Every answer other than "miopen" is a pass its engine takes — under the default switches, under each opt-in arithmetic with both
    dilated switches on, and under the A/B settings IPSR_BF16_ENGINES=all, IPSR_CONV_ENGINE=direct / winograd.  (Before `_select` /
    `_select_wrw` asked for W >= 4, Conv2d(k4, s1, p1) with >= 128 channels on 16..128 x 2 or 3 maps went to "wino_dil", which refuses
    extents below its kernel.)  And every engine of `_ENGINES` occurs: an engine that drops out of the grid cannot pass silently."""
    from deepinpainting_amd.models import hipconv
    refused, seen = sweep
    assert not refused, "%d selections are refused by the engine they name, first: %s" % (len(refused), refused[:6])
    assert set(e for e, _ in seen) == set(hipconv._ENGINES) - {"miopen"}, sorted(set(hipconv._ENGINES) - {"miopen"} - set(e for e, _ in seen))


@pytest.fixture
def hipconv(built, monkeypatch):
    """The dispatcher with no engine forced and no A/B switch set; restored afterwards."""
    from deepinpainting_amd.models import hipconv as hc
    monkeypatch.setattr(hc, "_FORCE", None)
    for var in _ENV_SWITCHES:
        monkeypatch.delenv(var, raising=False)
    hc.reload_env()
    yield hc
    monkeypatch.undo()
    hc.reload_env()


def test_envelope_rows_reach_the_engines_they_name(hipconv):
    """Under each row's switches `select` x 2 and `select_wrw` answer the row's triple, every pass on a HIP engine is one the engine takes,
    torch accepts the layer, and the row is as small as the table promises."""
    moved = []
    for row in de.ROWS:
        with de.switches(hipconv, row.switches):
            got = de.answers(hipconv, row.lay, row.bf16)
            ok = all(e == "miopen" or de.takes(e, kind, op, row.lay, row.bf16) for e, (kind, op) in zip(got, de.passes(row.lay)))
        if got != row.engines or not ok:
            moved.append((row.id, row.engines, got, ok))
        assert de.torch_accepts(row.lay) and row.H * row.W <= 16384, row.id
    assert not moved, "(row, expected, answered, the engines take it): %s" % (moved,)
    assert len(set(r.id for r in de.ROWS)) == len(de.ROWS)
    k4s1_below = [r for r in de.ROWS if r.geom == de.K4S1 and (r.cin, r.cout, r.H, r.W, r.B) == (128, 128, 16, 3, 1)]
    assert len(k4s1_below) == 1 and k4s1_below[0].engines == ("miopen",) * 3


# (engine, kind) whose rule admits one orientation only, and why
ONE_ORIENTATION = {}


def test_envelope_rows_cover_what_the_sweep_observes(sweep):
    """The (engine, kind) pairs of the table are exactly those the sweep observes; each pair has a row with H > W and one with H < W
    (`ONE_ORIENTATION` lists the rules that admit only one), one at batch 1 and one at batch 3."""
    _, seen = sweep
    have = {}
    for row in de.ROWS:
        for eng, (kind, _) in zip(row.engines, de.passes(row.lay)):
            if eng != "miopen":
                have.setdefault((eng, kind), []).append(row)
    assert set(have) == set(seen), (sorted(set(seen) - set(have)), sorted(set(have) - set(seen)))
    missing = []
    for pair, rows in sorted(have.items()):
        need = {"H > W": any(r.H > r.W for r in rows), "H < W": any(r.H < r.W for r in rows), "batch 1": any(r.B == 1 for r in rows), "batch 3": any(r.B == 3 for r in rows)}
        for orient in ONE_ORIENTATION.get(pair, {}):
            need.pop(orient)
        missing += [(pair, what) for what, ok in need.items() if not ok]
    assert not missing, missing
