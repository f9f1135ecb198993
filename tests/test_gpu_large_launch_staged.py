"""The staged entries and the filtered walk in the launch forms of 2,048 walks and more: granne_hip_search_postfiltered_batch*,
granne_hip_search_range_batch* and granne_hip_search_filtered_batch_device. tests/test_gpu_large_launch_entries.py holds
those forms to the oracle through every older entry; the three entries' own tests stop at 300, 96 and 256 queries, on
uniform data, with stage lists that hand no walk over. Here their stages are split launches (fast_kernel, then tail_kernel)
on the sketched 100-d index whose walks are handed over, launches that change form inside one call, chunks that share the
status words and the scratch block, exhausted containers, and the one-kernel forms with the id cache; the filtered walk
runs its plan for 4,096 walks and more.

The indexes, the form assertions and the output buffers are those of tests/test_gpu_large_launch_entries.py, imported; the
models are tests/postfilter_model.py and tests/range_model.py over those indexes' oracle graphs (inputs and caches:
tests/test_large_launch_staged_host.py, which also holds the preconditions on a machine without a GPU) and
tests/filter_model.py through tests/test_gpu_filtered.py's World. Every comparison is of the whole ids array, the distance
BYTES, counts, stage, found and status[3]; no tolerance anywhere; every test asserts the form that ran after the call.
Stages [50, 120, 250]: each lies just below the end of a register list of 64 S keys (S = 1, 2, 4), so a run of clones
across the list's end hands the walk over at every stage. What each test pins: tests/README_large_launch_staged.md."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import postfilter_model as pm  # noqa: E402
from tests import range_model as rm  # noqa: E402
from tests import test_large_launch_staged_host as host  # noqa: E402
from tests.test_gpu_filtered import worlds  # noqa: E402,F401  (the fixture: the filtered walk's indexes, queries and models)
from tests.test_gpu_large_launch_entries import (NQ, ODD, SLOW_SLOTS, Out, _form, _is_one_kernel, _is_oracles, _is_split, _stream,  # noqa: E402,F401
                                                 ga, world)  # (ga, world: the fixtures; world skips under the experiment knobs)

K, STAGES = host.K, host.STAGES
OUT_OF_REACH = 0xFFFFFFFF
COPIES = 17  # 17 x 256 = 4,352 walks: from 4,096 on the filtered plan halves the front table; no multiple of 64 S


def _p(x):
    return x.ctypes.data_as(C.c_void_p)


def _fb(fallback):
    """the entries' fallback code (GRANNE_HIP_PF_FALLBACK_* and _RG_FALLBACK_* are the same two numbers)"""
    from granne_amd import _lib
    assert (_lib.PF_FALLBACK_EXACT, _lib.PF_FALLBACK_SHORT) == (_lib.RG_FALLBACK_EXACT, _lib.RG_FALLBACK_SHORT)
    return _lib.PF_FALLBACK_EXACT if fallback == pm.EXACT else _lib.PF_FALLBACK_SHORT


def _the_form(gix, searched, what=None):
    """the form of a launch of `searched` walks on A"""
    (_is_split if searched >= NQ else _is_one_kernel)(gix, (what, searched))


def _last_searched(a):
    return [n for n in a.per_stage if n][-1]


def _mask_of(ga, world, case):
    key = ("filter", case.name)
    if key not in world.models:
        mask = host.band_mask(case.el)
        world.models[key] = (mask, ga.Filter.from_words(pm.words(mask), len(mask)))
    return world.models[key]


# ---- the post-filtered entries ---------------------------------------------------------------------------------------
def pf_device(ga, world, case, nq, min_allowed, stages, fallback, scratch_bytes=0, out=None, gix=None):
    """granne_hip_search_postfiltered_batch_device on the current stream: (ids, dists, counts, stage, status words), and
    the form of its last launch"""
    import torch
    gix = gix or case.gix
    f = _mask_of(ga, world, case)[1]
    dq = torch.from_numpy(case.q[:nq]).cuda()
    o = out or Out(nq, K, stats=False)
    stage = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
    gix.search_postfiltered_batch_device(dq.data_ptr(), nq, K, min_allowed, stages, _fb(fallback), f.ptr, 0, o.ids.data_ptr(), o.ds.data_ptr(),
                                         o.cnt.data_ptr(), stage.data_ptr(), o.status.data_ptr(), scratch_bytes, _stream())
    form = _form(gix)
    torch.cuda.synchronize()
    return o.host() + (stage.cpu().numpy().view(np.uint32), o.words()), form


def pf_host(ga, world, case, nq, min_allowed, stages, fallback, scratch_bytes=0):
    """granne_hip_search_postfiltered_batch: its return code, then as pf_device"""
    from granne_amd import _lib
    mask = _mask_of(ga, world, case)[0]
    q = np.ascontiguousarray(case.q[:nq])
    ids, ds = np.zeros((nq, K), np.uint64), np.zeros((nq, K), np.float32)
    cnt, stage, st = np.full(nq, 77, np.uint32), np.full(nq, 77, np.uint32), np.full(4, 9, np.uint32)
    rc = _lib.lib().granne_hip_search_postfiltered_batch(case.gix._h, _p(q), nq, K, min_allowed, (C.c_uint32 * len(stages))(*stages), len(stages),
                                                         _fb(fallback), _p(pm.words(mask)), 0, scratch_bytes, _p(ids), _p(ds), _p(cnt),
                                                         _p(stage), _p(st))
    return rc, (ids, ds, cnt, stage, st.tolist()), _form(case.gix)


def pf_is_model(got, a, what=None):
    ids, ds, cnt, stage, st = got
    assert (stage == a.stage).all(), (what, np.nonzero(stage != a.stage)[0][:5])
    assert (cnt == a.counts).all(), what
    bad = np.nonzero((ids != a.ids).any(axis=1))[0]
    assert bad.size == 0, (what, bad[:5], ids[bad[:1]], a.ids[bad[:1]], a.stage[bad[:5]])
    assert ds.tobytes() == a.dists.tobytes(), what
    assert st[0] == 0 and st[3] == a.unfinished, (what, st, a.unfinished)


def pf_call(entry, ga, world, case, nq, min_allowed, stages, fallback):
    from granne_amd import _lib
    if entry == "device":
        return pf_device(ga, world, case, nq, min_allowed, stages, fallback)
    rc, got, form = pf_host(ga, world, case, nq, min_allowed, stages, fallback)
    assert rc == _lib.OK
    return got, form


# ---- the range entries -----------------------------------------------------------------------------------------------
def rg_device(case, nq, radii, cap, stages, fallback, scratch_bytes=0, out=None, gix=None):
    """granne_hip_search_range_batch_device on the current stream: (ids, dists, counts, found, stage, status words), and
    the form of its last launch"""
    import torch
    gix = gix or case.gix
    dq, dr = torch.from_numpy(case.q[:nq]).cuda(), torch.from_numpy(radii).cuda()
    o = out or Out(nq, cap, stats=False)
    found, stage = (torch.full((nq,), 77, dtype=torch.int32, device="cuda") for _ in range(2))
    gix.search_range_batch_device(dq.data_ptr(), nq, dr.data_ptr(), cap, stages, _fb(fallback), o.ids.data_ptr(), o.ds.data_ptr(),
                                  o.cnt.data_ptr(), found.data_ptr(), stage.data_ptr(), o.status.data_ptr(), scratch_bytes, _stream())
    form = _form(gix)
    torch.cuda.synchronize()
    return o.host() + (found.cpu().numpy().view(np.uint32), stage.cpu().numpy().view(np.uint32), o.words()), form


def rg_host(case, nq, radii, cap, stages, fallback, scratch_bytes=0):
    from granne_amd import _lib
    q = np.ascontiguousarray(case.q[:nq])
    ids, ds = np.zeros((nq, cap), np.uint64), np.zeros((nq, cap), np.float32)
    cnt, found, stage, st = np.full(nq, 77, np.uint32), np.full(nq, 77, np.uint32), np.full(nq, 77, np.uint32), np.full(4, 9, np.uint32)
    rc = _lib.lib().granne_hip_search_range_batch(case.gix._h, _p(q), nq, _p(radii), cap, (C.c_uint32 * len(stages))(*stages), len(stages),
                                                  _fb(fallback), scratch_bytes, _p(ids), _p(ds), _p(cnt), _p(found), _p(stage), _p(st))
    return rc, (ids, ds, cnt, found, stage, st.tolist()), _form(case.gix)


def rg_is_model(got, a, what=None):
    ids, ds, cnt, found, stage, st = got
    assert (stage == a.stage).all(), (what, np.nonzero(stage != a.stage)[0][:5])
    assert (found == a.found).all(), (what, np.nonzero(found != a.found)[0][:5])
    assert (cnt == a.counts).all(), what
    bad = np.nonzero((ids != a.ids).any(axis=1))[0]
    assert bad.size == 0, (what, bad[:5], ids[bad[:1]], a.ids[bad[:1]])
    assert ds.tobytes() == a.dists.tobytes(), what
    assert st[0] == 0 and st[3] == a.unfinished, (what, st, a.unfinished)


# ---- 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("fallback", [pm.EXACT, pm.SHORT])
def test_postfiltered_on_the_tied_index(ga, world, fallback, entry):
    """8,192 queries of A "clones" under one filter whose density varies by band, k = 10. min_allowed 40: every outcome,
    all three stages split launches. A one-stage call [50] of all 8,192: split. min_allowed 24: the last stage falls below
    the threshold, so the call ends in the one-kernel form. All three are the model's."""
    case = world.tied()
    a, s, few = host.pf_preconditions(world, case)
    for min_allowed, stages in ((host.MIN_ALLOWED, STAGES[:1]), (host.MIN_ALLOWED, STAGES), (host.MIN_ALLOWED_FEW, STAGES)):
        m = host.pf_model(world, case, host.PF_NQ, min_allowed, stages, fallback)
        got, form = pf_call(entry, ga, world, case, host.PF_NQ, min_allowed, stages, fallback)
        print("post-filtered", fallback, entry, min_allowed, stages, "per stage", m.per_stage, "outcomes", m.outcome_counts(len(stages)), "form", form)
        _the_form(case.gix, _last_searched(m), (min_allowed, stages))
        pf_is_model(got, m, (fallback, entry, min_allowed, stages))
    assert _last_searched(few) <= NQ - host.MARGIN and _last_searched(a) >= NQ + host.MARGIN  # (both forms were asserted above)


# ---- 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", host.CAPS)
@pytest.mark.parametrize("fallback", [rm.EXACT, rm.SHORT])
def test_range_on_the_tied_index(world, oracle, fallback, cap):
    """4,200 queries of A "clones" under the exact radii (the distance to the 3rd / 40th / 200th / 900th neighbour, -0.5,
    +inf), many of them inside a run of clones: stages 0 and 1 are split launches, stage 2 one kernel -- each asserted after
    a call whose stage list ends there. cap 3 lies below the lists, 50 between them, 1024 above all. The host entry at cap 50."""
    case = world.tied()
    radii = host.exact_radii(oracle, case, host.RG_NQ)
    assert host.radii_inside_runs(oracle, case, host.RG_NQ) >= 64
    a = host.rg_preconditions(world, case, fallback, cap)
    for n in (1, 2, 3):
        m = host.rg_model(world, case, host.RG_NQ, radii, cap, STAGES[:n], fallback)
        assert m.per_stage == a.per_stage[:n]
        got, form = rg_device(case, host.RG_NQ, radii, cap, STAGES[:n], fallback)
        print("range", fallback, cap, STAGES[:n], "per stage", m.per_stage, "fallback", m.unfinished, "form", form)
        _the_form(case.gix, m.per_stage[-1], (cap, n))
        rg_is_model(got, m, (fallback, cap, n))
    if cap == 50:
        from granne_amd import _lib
        rc, got, form = rg_host(case, host.RG_NQ, radii, cap, STAGES, fallback)
        assert rc == _lib.OK
        _the_form(case.gix, a.per_stage[-1], "host")
        rg_is_model(got, a, (fallback, "host"))


# ---- 3 ---------------------------------------------------------------------------------------------------------------
def test_the_threshold_inside_a_call(ga, world):
    """Stage 0 of 2,047, 2,048 and 2,049 queries -- one kernel, split, split, asserted after a one-stage call -- and later
    stages below the threshold: the three-stage call changes form inside and is the model's. Then all 8,192 with
    scratch_bytes for chunks of 1,024 and of 2,048 first-stage lists (fewer of the later stages' longer lists): launches
    above and below the threshold in one call, the same bytes for any value."""
    case = world.tied()
    for n in (NQ - 1, NQ, NQ + 1):
        one = host.pf_model(world, case, n, host.MIN_ALLOWED, STAGES[:1], pm.SHORT)
        got, _ = pf_device(ga, world, case, n, host.MIN_ALLOWED, STAGES[:1], pm.SHORT)
        _the_form(case.gix, n, "one stage")
        pf_is_model(got, one, ("one stage", n))
        m = host.pf_model(world, case, n, host.MIN_ALLOWED_FEW, STAGES, pm.EXACT)
        assert 0 < m.per_stage[1] < NQ and 0 < m.per_stage[2] < NQ, m.per_stage
        got, _ = pf_device(ga, world, case, n, host.MIN_ALLOWED_FEW, STAGES, pm.EXACT)
        _is_one_kernel(case.gix, n)
        pf_is_model(got, m, n)
    a = host.pf_model(world, case, host.PF_NQ, host.MIN_ALLOWED, STAGES, pm.EXACT)
    one = host.pf_model(world, case, host.PF_NQ, host.MIN_ALLOWED, STAGES[:1], pm.SHORT)
    for lists in (1024, 2048):
        scratch = lists * 12 * STAGES[0]
        got, _ = pf_device(ga, world, case, host.PF_NQ, host.MIN_ALLOWED, STAGES[:1], pm.SHORT, scratch_bytes=scratch)
        _the_form(case.gix, lists, "chunks")  # (8,192 is a multiple of both: the last chunk is a whole one)
        pf_is_model(got, one, ("one stage, chunks of", lists))
        got, _ = pf_device(ga, world, case, host.PF_NQ, host.MIN_ALLOWED, STAGES, pm.EXACT, scratch_bytes=scratch)
        _is_one_kernel(case.gix, lists)  # (a chunk of the last stage holds lists * 50 / 250 lists)
        pf_is_model(got, a, ("chunks of", lists))


# ---- 4 ---------------------------------------------------------------------------------------------------------------
def _staged(which, ga, world, oracle, case):
    """(the model's answer, call(scratch_bytes=0, out=None, gix=None) -> (got, form), is_model) of the module's main call
    through the post-filtered or the range device entry"""
    if which == "postfiltered":
        a = host.pf_model(world, case, host.PF_NQ, host.MIN_ALLOWED, STAGES, pm.EXACT)
        return a, lambda **kw: pf_device(ga, world, case, host.PF_NQ, host.MIN_ALLOWED, STAGES, pm.EXACT, **kw), pf_is_model
    radii = host.exact_radii(oracle, case, host.RG_NQ)
    a = host.rg_model(world, case, host.RG_NQ, radii, 50, STAGES, rm.EXACT)
    return a, lambda **kw: rg_device(case, host.RG_NQ, radii, 50, STAGES, rm.EXACT, **kw), rg_is_model


def _handed_over_by_the_plain_entry(world, case, a, which):
    """The sum, over the model's per-stage pending sets, of last_slow_count() after search_batch(q[pending_s], E_s, E_s)
    on the case's handle: the plain entry, which the large-launch module holds to the oracle (as it is here)."""
    key = ("handed", which)
    if key not in world.models:
        per_stage = []
        for E, pend in zip(STAGES, host.pending_sets(a, len(STAGES))):
            q = np.ascontiguousarray(case.q[pend])
            got = case.gix.search_batch(q, E, E, stats=True)
            per_stage.append(case.gix.last_slow_count())
            _the_form(case.gix, len(pend), ("plain", E))
            _is_oracles(got, case.oix.search_batch(q, E, E), slice(None), ("plain", which, E))
        print(which, "hand-overs per stage", per_stage, "of", [len(p) for p in host.pending_sets(a, len(STAGES))])
        world.models[key] = per_stage
    return world.models[key]


@pytest.mark.parametrize("which", ["postfiltered", "range"])
def test_hand_overs_are_counted(ga, world, oracle, which):
    """status[1] of the device entries, into zeroed words, is what the plain entry hands over on the same pending sets; it
    is positive (the module's premise: the stages' tail kernels have lists to walk), unchanged under chunking, and doubles
    when the call is made twice into the same words, as status[3] does; status[0] stays 0."""
    case = world.tied()
    a, call, is_model = _staged(which, ga, world, oracle, case)
    per_stage = _handed_over_by_the_plain_entry(world, case, a, which)
    total = sum(per_stage)
    assert total > 0 and min(per_stage) > 0, per_stage  # (every stage's tail kernel has lists to walk)
    got, _ = call()
    is_model(got, a, which)
    assert got[-1][:2] == [0, total] and got[-1][3] == a.unfinished, (got[-1], per_stage, a.unfinished)
    got, _ = call(scratch_bytes=1024 * 12 * STAGES[0])
    is_model(got, a, (which, "chunks"))
    assert got[-1][:2] == [0, total] and got[-1][3] == a.unfinished, (got[-1], per_stage, a.unfinished)
    o = Out(len(a.counts), got[0].shape[1], stats=False)
    call(out=o)
    got, _ = call(out=o)
    assert got[-1][:2] == [0, 2 * total] and got[-1][3] == 2 * a.unfinished, (got[-1], per_stage, a.unfinished)


# ---- 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["uniform", "b200", "b96"])
def test_uniform_data_and_the_one_kernel_forms(ga, world, which):
    """A "uniform" (2,500 queries: a split first stage with nothing to hand over) and B 200-d / 96-d (2,048: one kernel with
    the id cache, the unrolled and the streamed walker), post-filtered (min_allowed 24, the exact fallback) and range (radii
    from the oracle's walk, the short fallback) once each. On B the same call with GRANNE_HIP_OPT_SEEN_MIN out of reach --
    no id cache -- gives the same bytes in the same form."""
    from granne_amd import _lib
    case, nq = (world.a("uniform"), ODD) if which == "uniform" else (world.b(int(which[1:])), NQ)
    gix = case.gix
    a = host.pf_model(world, case, nq, host.MIN_ALLOWED_FEW, STAGES, pm.EXACT)
    radii = host.walk_radii(world, case, nq, STAGES)
    g = host.rg_model(world, case, nq, radii, 50, STAGES, rm.SHORT)
    assert a.per_stage[0] >= NQ and min(a.per_stage) >= host.MARGIN and g.per_stage[0] >= NQ, (a.per_stage, g.per_stage)
    assert set(g.stage.tolist()) == {0, 1, 2, rm.STAGE_SHORT}
    print(which, "post-filtered per stage", a.per_stage, "outcomes", a.outcome_counts(3), "range per stage", g.per_stage)

    def form(searched, what):
        if which == "uniform":
            _the_form(gix, searched, what)
        else:
            _is_one_kernel(gix, what)

    if which == "uniform":  # the first stage's form, by a call that ends there
        one = host.pf_model(world, case, nq, host.MIN_ALLOWED_FEW, STAGES[:1], pm.SHORT)
        got, _ = pf_device(ga, world, case, nq, host.MIN_ALLOWED_FEW, STAGES[:1], pm.SHORT)
        _is_split(gix, "uniform, one stage")
        pf_is_model(got, one, "uniform, one stage")
    pf, _ = pf_device(ga, world, case, nq, host.MIN_ALLOWED_FEW, STAGES, pm.EXACT)
    form(_last_searched(a), "post-filtered")
    pf_is_model(pf, a, which)
    rg, _ = rg_device(case, nq, radii, 50, STAGES, rm.SHORT)
    form(g.per_stage[-1], "range")
    rg_is_model(rg, g, which)
    if which != "uniform":
        gix.set_option(_lib.OPT_SEEN_MIN, OUT_OF_REACH)
        try:
            pf2, _ = pf_device(ga, world, case, nq, host.MIN_ALLOWED_FEW, STAGES, pm.EXACT)
            _is_one_kernel(gix, "post-filtered, no id cache")
            rg2, _ = rg_device(case, nq, radii, 50, STAGES, rm.SHORT)
            _is_one_kernel(gix, "range, no id cache")
        finally:
            gix.set_option(_lib.OPT_SEEN_MIN, NQ)
        for x, y in zip(pf[:4] + rg[:5], pf2[:4] + rg2[:5]):
            assert x.tobytes() == y.tobytes(), which
        assert pf2[4] == pf[4] and rg2[5] == rg[5]


# ---- 6 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["postfiltered", "range"])
def test_exhaustion_through_a_stage(ga, world, oracle, which):
    """GRANNE_HIP_OPT_FORCE_SLOW with 256 containers: every walk of a one-stage [200] call of 2,048 queries outgrows them.
    The host entry returns GRANNE_HIP_ERR_OVERFLOW, the device entry leaves status[0] != 0 (nothing is asserted about the
    voided rows). With the options restored the same handle answers the three-stage call as the model and counts the
    hand-overs of a fresh handle: the control words were re-armed after the exhausted launches."""
    from granne_amd import _lib
    case = world.tied()
    gix = case.gix
    a, call, is_model = _staged(which, ga, world, oracle, case)
    fresh = ga.Granne("angular", case.el, case.oix.layers)
    try:
        fresh.set_option(_lib.OPT_SLOW_SLOTS, SLOW_SLOTS)
        got, _ = call(gix=fresh)
        _the_form(fresh, _last_searched(a), "fresh")
        is_model(got, a, (which, "fresh"))
        first = got[-1]
    finally:
        fresh.close()
    assert first[0] == 0 and first[1] > 0, first
    radii = host.exact_radii(oracle, case, host.RG_NQ)[:NQ] if which == "range" else None
    slots = gix.get_option(_lib.OPT_SLOW_SLOTS)
    try:
        gix.set_option(_lib.OPT_FORCE_SLOW, 1)
        gix.set_option(_lib.OPT_SLOW_SLOTS, 256)
        if which == "postfiltered":
            rc, _, _ = pf_host(ga, world, case, NQ, host.MIN_ALLOWED, [200], pm.SHORT)
        else:
            rc, _, _ = rg_host(case, NQ, radii, 50, [200], rm.SHORT)
        assert rc == _lib.ERR_OVERFLOW, (rc, _lib.lib().granne_hip_last_error())
        _is_split(gix, "exhausted, host entry", forced=True)
        if which == "postfiltered":
            got, _ = pf_device(ga, world, case, NQ, host.MIN_ALLOWED, [200], pm.SHORT)
        else:
            got, _ = rg_device(case, NQ, radii, 50, [200], rm.SHORT)
        _is_split(gix, "exhausted, device entry", forced=True)
        assert got[-1][0] != 0, got[-1]
    finally:
        gix.set_option(_lib.OPT_FORCE_SLOW, 0)
        gix.set_option(_lib.OPT_SLOW_SLOTS, slots)
    got, _ = call()
    _the_form(gix, _last_searched(a), "restored")
    is_model(got, a, (which, "restored"))
    assert got[-1][:2] == first[:2] and got[-1][3] == first[3], (got[-1], first)


# ---- 7 ---------------------------------------------------------------------------------------------------------------
FILTERED = [(name, ms, kind) for name in ("f32_d100", "i8_d32") for ms in (100, 200) for kind in (1.0, 0.2)]
FILTERED += [("f32_d100", 100, "per_query"), ("i8_d32", 100, "per_query")]


@pytest.mark.parametrize("name,ms,kind", FILTERED)
def test_the_filtered_walk_at_4352_walks(ga, worlds, name, ms, kind):  # noqa: F811
    """The 256 queries of tests/test_gpu_filtered.py's worlds 17 times in one launch, blocked (walkers next to each other
    share a query) and interleaved (they do not), the per-query filters repeated alike: every copy's ids, distance bytes,
    counts and counters are the model's row for its query, status[3] is 17 times the model's cut count (0 without
    max_expand), status[1] 17 times the 256-query launch's, status[0] is 0. From 4,096 walks on the plan halves the front
    table for max_search >= 65; status[2], the walks that borrowed an overflow table, is printed, not asserted."""
    import torch
    from granne_amd import _lib
    from tests import filter_model as fm
    w = worlds(name)
    k, nq = ms + 5, COPIES * 256
    mi, md, mc, mst, cut = w.model(kind, ms)
    base = w.check(kind, ms, k)  # the 256-query launch is the model's; its status words
    assert w.gix.get_option(_lib.OPT_LAST_WALKER) == _lib.WALKER_GENERAL and int(base[0]) == 0
    allowed = w.allowed(kind)
    words = torch.from_numpy(np.stack([fm.pack_bits(row) for row in allowed]).view(np.int32)).cuda()
    for order, at in (("blocked", np.arange(nq) // COPIES), ("interleaved", np.arange(nq) % 256)):
        dq = torch.from_numpy(np.ascontiguousarray(w.q[at])).cuda()
        if len(allowed) > 1:
            dwords, stride = words[torch.from_numpy(at).cuda()].contiguous(), words.shape[1]
        else:
            dwords, stride = words, 0
        o = Out(nq, k)
        w.gix.search_filtered_batch_device(dq.data_ptr(), nq, ms, k, dwords.data_ptr(), stride, 0, *o.args(), _stream())
        assert w.gix.get_option(_lib.OPT_LAST_WALKER) == _lib.WALKER_GENERAL
        torch.cuda.synchronize()
        ids, ds, cnt, st = o.host()
        st4 = o.words()
        print("filtered", name, ms, kind, order, "status of 256:", [int(x) for x in base], "of", nq, ":", st4)
        assert (cnt == mc[at]).all(), order
        assert (ids == mi[at]).all(), (order, np.nonzero((ids != mi[at]).any(axis=1))[0][:5])
        assert ds.tobytes() == np.ascontiguousarray(md[at]).tobytes(), order
        assert (st == mst[at]).all(), (order, np.nonzero((st != mst[at]).any(axis=1))[0][:5])
        assert st4[0] == 0 and st4[1] == COPIES * int(base[1]) and st4[3] == COPIES * int(cut.sum()), (order, st4, base)
