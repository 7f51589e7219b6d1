"""The dispatcher of models/hipconv.py at the edges of what its rules admit — host logic and workspace probes only, no kernel is launched.

The rules were measured on square maps at batch 8 / 16, and several bound H alone, or H * W alone, and channel counts from below only: they
hand the engines elongated maps, one-row and one-column maps and other batches.  The checks:
  * every answer of the sweep is the recorded one (digests per block, tests/golden/dispatch_envelope_digests.json); the two dilated switches
    for bf16 activations move no block of fp32 activations, of IPSR_BF16_ENGINES=all or of another geometry;
  * `hipconv.engine_takes`, what the rules and the final guard ask, equals the independent restatement `dispatch_envelope.takes`; an engine
    whose record refuses is never answered; the direct opt-in switches (the arithmetic name and the four dilated booleans) build one set;
  * no answer of `select` / `select_wrw` over a grid with H != W is one the chosen engine's own support query refuses (such a layer would
    raise NotImplementedError in `conv_nobias` although torch computes it);
  * every row of tests/dispatch_envelope.py's corner table still reaches the engines it names (tests/test_gpu_dispatch_envelope.py runs
    those rows against fp64: a row whose answer moved to MIOpen would compare MIOpen with fp64 and pass);
  * the table covers every (engine, pass kind) the grid observes, in both orientations and at batches 1 and 3.
"""
import hashlib
import json
import os
from collections import namedtuple

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
            ("engine_winograd", {"IPSR_CONV_ENGINE": "winograd"}, "default", (False, True), CHANNELS),
            # the two dilated switches for bf16 activations (de.BF16_DIL_SWITCHES): each alone and both; both under fp32 activations, which they
            # must not move; both under IPSR_BF16_ENGINES=all, where the opt-ins stand down
            ("bf16_dil_data", {}, "bf16_dil_data", (True,), CHANNELS), ("bf16_dil_dw", {}, "bf16_dil_dw", (True,), CHANNELS),
            ("bf16_dil", {}, "bf16_dil", (False, True), CHANNELS),
            ("bf16_all_dil", {"IPSR_BF16_ENGINES": "all"}, "bf16_dil", (True,), CHANNELS)]
assert CHANNELS_DEFAULT[:len(CHANNELS)] == CHANNELS      # `Sweep.common` compares the settings over their common channel pairs, the leading ones
_ENV_SWITCHES = ("IPSR_CONV_ENGINE", "IPSR_NO_SMALLMAP", "IPSR_NO_THIN", "IPSR_SMALLMAP_MAX_POS", "IPSR_BF16_ENGINES")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from deepinpainting_amd import _lib
    return _lib


# ---- every answer of the sweep, pinned by digest ---------------------------------------------------------------------------------------
# tests/golden/dispatch_envelope_digests.json holds one SHA-256 and one answer count per block of the sweep, block = (setting, dtype, batch,
# geometry): the digest of the block's answers, "miopen" included, one character each (the engine's index in `DIGEST_ENGINES`, base 36), in
# the order the sweep walks — channels x H x W x Conv2d / ConvTranspose2d x (forward, input gradient, weight gradient), shapes torch refuses
# left out.  tests/golden/engine_selection.json.gz pins square maps under the default arithmetic; this pins the elongated maps and the opt-in
# arithmetics.  A pull request that re-routes or widens an engine regenerates the file
# (IPSR_REGENERATE_DISPATCH_DIGESTS=1 python -m pytest tests/test_dispatch_envelope.py -k recorded_digests) and shows which blocks moved; one
# that only restructures the rules must never regenerate it from the restructured code.
DIGEST_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dispatch_envelope_digests.json")
DIGEST_ENGINES = ["miopen", "winograd", "wino_dil", "wino_s2", "thin", "thin_f2m", "thin_mfma", "smallmap", "direct", "one", "bf16d", "bf16x3d", "bf16x3w"]
_DIGITS = "0123456789abcdefghijklmnopqrstuvwxyz"

Sweep = namedtuple("Sweep", "refused seen blocks disagree common")


def _block_key(setting, bf16, B, geom):
    return "%s/%s/b%d/k%ds%dp%dd%d" % ((setting, "bf16" if bf16 else "fp32", B) + tuple(geom))


@pytest.fixture(scope="module")
def swept(built):
    """-> Sweep over settings x dtypes x batches x geometries x channels x H x W x the three passes of Conv2d and of ConvTranspose2d, on the
    shapes torch accepts:
      refused   the answers the chosen engine's own support query (`de.takes`) refuses, as (setting, engine, kind, op, lay, bf16)
      seen      {(engine, kind): count} of every answer other than "miopen"
      blocks    {block key: (SHA-256 of the block's answers, their count)}, see `DIGEST_FIXTURE`
      disagree  the answers on which `hipconv.engine_takes` and `de.takes` differ, as `refused` (None under a hipconv.py from before the engine
                records had `takes`: the digests can be checked against such a file, nothing else here can)
      common    {block key: SHA-256 of the block's answers over the channel pairs of `CHANNELS`}, the leading pairs of every setting: what two
                settings swept with different channel lists are compared by"""
    from deepinpainting_amd import ops
    from deepinpainting_amd.models import hipconv
    assert sorted(n for n, _, sw, _, _ in SETTINGS if sw != "default" and sw not in de.BF16_DIL_SWITCHES) == sorted(ops.DIRECT_PASSES)
    code = {e: _DIGITS[i] for i, e in enumerate(DIGEST_ENGINES)}
    engine_takes = getattr(hipconv, "engine_takes", None)
    mp = pytest.MonkeyPatch()
    refused, seen, points, blocks, disagree, common = [], {}, 0, {}, None if engine_takes is None else [], {}
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
                            key, chars = _block_key(name, bf16, B, geom), []
                            for n, (Cin, Cout) in enumerate(channels):
                                if n == len(CHANNELS):
                                    common[key] = hashlib.sha256("".join(chars).encode("ascii")).hexdigest()
                                for H in EXTENTS:
                                    for W in EXTENTS:
                                        for transposed in (False, True):
                                            lay = (transposed, B, Cin, H, W, Cout) + geom
                                            if not de.torch_accepts(lay):
                                                continue
                                            for eng, (kind, op) in zip(de.answers(hipconv, lay, bf16), de.passes(lay)):
                                                points += 1
                                                chars.append(code[eng])
                                                if eng == "miopen":
                                                    continue
                                                seen[(eng, kind)] = seen.get((eng, kind), 0) + 1
                                                took = de.takes(eng, kind, op, lay, bf16)
                                                if not took:
                                                    refused.append((name, eng, kind, op, lay, bf16))
                                                if engine_takes is not None and engine_takes(eng, kind, op, lay, bf16) != took:
                                                    disagree.append((name, eng, kind, op, lay, bf16))
                            blocks[key] = (hashlib.sha256("".join(chars).encode("ascii")).hexdigest(), len(chars))
                            common.setdefault(key, blocks[key][0])
                    hipconv._SEL.clear()             # the memo of a finished dtype is dead weight
    finally:
        mp.undo()
        hipconv.reload_env()
    print("dispatcher sweep: %d answers, %d on a HIP engine, %d refused" % (points, sum(seen.values()), len(refused)))
    return Sweep(refused, seen, blocks, disagree, common)


@pytest.fixture(scope="module")
def sweep(swept):
    """-> (refused, seen) of `swept`."""
    return swept.refused, swept.seen


def test_sweep_answers_match_the_recorded_digests(swept):
    """Every answer of the sweep, "miopen" included, is the one recorded: per block (setting, dtype, batch, geometry) the digest and the count
    of the answers equal the fixture's.  `test_no_selection_is_refused_by_its_engine` checks that answers are taken, not what they are;
    this pins what they are, on elongated maps and under every opt-in arithmetic."""
    if os.environ.get("IPSR_REGENERATE_DISPATCH_DIGESTS") == "1":
        doc = {"engines": DIGEST_ENGINES, "extents": EXTENTS, "order": "per block: channels x H x W x (Conv2d, ConvTranspose2d) x (forward, input gradient, "
               "weight gradient), shapes torch refuses left out; one base-36 digit per answer, its index in `engines`",
               "blocks": {key: {"sha256": sha, "answers": n} for key, (sha, n) in swept.blocks.items()}}
        with open(DIGEST_FIXTURE, "w") as f:
            json.dump(doc, f, sort_keys=True, indent=0)
            f.write("\n")
    with open(DIGEST_FIXTURE) as f:
        doc = json.load(f)
    assert doc["engines"] == DIGEST_ENGINES and doc["extents"] == EXTENTS
    want = {key: (b["sha256"], b["answers"]) for key, b in doc["blocks"].items()}
    assert sorted(want) == sorted(swept.blocks), (sorted(set(want) - set(swept.blocks)), sorted(set(swept.blocks) - set(want)))
    moved = sorted(key for key in want if want[key] != swept.blocks[key])
    assert not moved, "%d of %d blocks moved (block: recorded count -> now): %s" % (
        len(moved), len(want), ", ".join("%s: %d -> %d" % (k, want[k][1], swept.blocks[k][1]) for k in moved))
    assert sum(n for _, n in want.values()) > 1000000 and len(want) >= 300


def test_bf16_dilated_switches_move_nothing_else(swept):
    """What the two dilated switches for bf16 activations must leave alone, block against block over the channel pairs of `CHANNELS`: fp32
    activations (both on: the "default" answers); IPSR_BF16_ENGINES=all (both on: the "bf16_all" answers, the opt-ins stand down under any
    value of that variable); and, under each of the three switch names, every geometry but the dilated one (the "default" answers)."""
    moved = []
    for B in BATCHES:
        for geom in GEOMS:
            same = [(("bf16_dil", False), ("default", False)), (("bf16_all_dil", True), ("bf16_all", True))]
            same += [((name, True), ("default", True)) for name in de.BF16_DIL_SWITCHES if geom != de.DIL]
            for (a, a16), (b, b16) in same:
                ka, kb = _block_key(a, a16, B, geom), _block_key(b, b16, B, geom)
                if swept.common[ka] != swept.common[kb]:
                    moved.append((ka, kb))
    assert not moved, moved
    # ... and the dilated blocks do move under each name, or the comparison above compares nothing
    assert all(swept.common[_block_key(name, True, 8, de.DIL)] != swept.common[_block_key("default", True, 8, de.DIL)] for name in de.BF16_DIL_SWITCHES)


def test_engine_takes_is_the_independent_restatement(swept, hipconv):
    """`hipconv.engine_takes` — the `takes` of the engine records, what the rules and the final guard ask — equals `de.takes`, the restatement
    by geometry in tests/dispatch_envelope.py: for the answered engine at every point of the sweep, and for every engine x the three passes on
    every row of the corner table, with the row's dtype and with the other one.  "miopen" takes everything."""
    assert swept.disagree == [], "%d sweep answers, first: %s" % (len(swept.disagree), swept.disagree[:6])
    differ = []
    for row in de.ROWS:
        with de.switches(hipconv, row.switches):
            for bf16 in (row.bf16, not row.bf16):
                for kind, op in de.passes(row.lay):
                    assert hipconv.engine_takes("miopen", kind, op, row.lay, bf16) is True
                    for eng in hipconv._ENGINES:
                        if eng != "miopen" and hipconv.engine_takes(eng, kind, op, row.lay, bf16) != de.takes(eng, kind, op, row.lay, bf16):
                            differ.append((row.id, eng, kind, op, bf16))
    assert not differ, differ


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


def test_an_engine_that_refuses_is_never_answered(hipconv):
    """The final guard of `_select_any` / `_select_wrw_any`: with one record's `takes` answering False, no pass of any row of the corner table
    is answered with that engine — it goes to "miopen" or to a later rule's engine — and the passes of the other engines stay.  "winograd" and
    "wino_dil" are the engines whose rules probe nothing, "wino_s2" probes for its data passes only, "smallmap" probes in its rule."""
    for refused in ("winograd", "wino_dil", "wino_s2", "smallmap"):
        rows = [r for r in de.ROWS if refused in r.engines]
        assert rows, refused
        for patched in (True, False):            # then with the record put back: the rows answer their engines again
            with pytest.MonkeyPatch.context() as mp:
                if patched:
                    mp.setitem(hipconv._ENGINES, refused, hipconv._ENGINES[refused]._replace(takes=lambda kind, op, lay, bf16: False))
                hipconv._SEL.clear()
                try:
                    for row in rows:
                        with de.switches(hipconv, row.switches):
                            got = de.answers(hipconv, row.lay, row.bf16)
                        assert not patched or refused not in got, (refused, row.id, got)
                        assert all(g == e for g, e in zip(got, row.engines) if not patched or e != refused), (refused, row.id, got)
                finally:
                    hipconv._SEL.clear()


def test_direct_switches_build_one_set(hipconv):
    """`_direct_passes_on` over the 2^4 x 5 settings of the four dilated booleans and the fp32 arithmetic: the passes of ops.DIRECT_PASSES
    for the name plus one key per boolean that is on, and the four public getters read the same set.  The direct names stay refused for
    bf16 activations."""
    from deepinpainting_amd import ops
    setters = {"dil_data": hipconv.set_direct_dilated, "dil_wrw": hipconv.set_direct_dilated_dw,
               "bf16_dil_data": hipconv.set_direct_dilated_bf16, "bf16_dil_wrw": hipconv.set_direct_dilated_bf16_dw}
    getters = {"dil_data": hipconv.direct_dilated, "dil_wrw": hipconv.direct_dilated_dw,
               "bf16_dil_data": hipconv.direct_dilated_bf16, "bf16_dil_wrw": hipconv.direct_dilated_bf16_dw}
    was = (hipconv._MATH["fp32"], {key: get() for key, get in getters.items()})
    try:
        for math in ["fp32"] + sorted(ops.DIRECT_PASSES):
            for bits in range(16):
                on = {key: bool(bits >> i & 1) for i, key in enumerate(setters)}
                hipconv.set_conv_math(fp32=math)
                for key, val in on.items():
                    setters[key](val)
                want = set(ops.DIRECT_PASSES.get(math, ())) | set(key for key, val in on.items() if val)
                assert set(hipconv._direct_passes_on()) == want, (math, on)
                assert (hipconv._MATH["fp32"], {key: get() for key, get in getters.items()}) == (math, on)
                assert all(get() is on[key] for key, get in getters.items())
                assert all(ops.direct_moves(math, key) == (key in want) for key in ("k3_data", "k3_wrw", "s2_data", "s2_wrw"))
        assert set(r.key for r in hipconv._DIRECT_OPT_INS) == set().union(*ops.DIRECT_PASSES.values()) | set(setters)
        for name in ops.DIRECT_PASSES:
            with pytest.raises(ValueError):
                hipconv.set_conv_math(bf16=name)
        assert hipconv._MATH["bf16"] not in ops.DIRECT_PASSES
    finally:
        hipconv.set_conv_math(fp32=was[0])
        for key, val in was[1].items():
            setters[key](val)


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
