"""The preconditions of tests/test_gpu_large_launch_staged.py that need only the oracle and the models, and the inputs both
modules share: the stage list, the filter, the radii, the cached model answers. What each test pins:
tests/README_large_launch_staged.md.

The indexes are those of tests/test_gpu_large_launch_entries.py, made by its World -- here over handles that hold nothing,
so that the module runs without a GPU. A graph built by eight threads may differ from run to run, so every condition is a
margin, none a pinned number; the model answers are kept on the World that owns the graph they were walked on."""
import numpy as np

from tests import postfilter_model as pm
from tests import range_model as rm
from tests import test_gpu_large_launch_entries as lle

NQ = lle.NQ
STAGES = [50, 120, 250]  # each just below the end of a register list of 64 S keys: S = 1 up to 60, 2 up to 124, 4 up to 252
SLOTS = [1, 2, 4]
K = lle.K
PF_NQ = 4 * NQ   # the post-filtered launch: A "clones"' whole pool
RG_NQ = 4200     # the range launch: stages 0 and 1 at or above the threshold, stage 2 below it
TIE_NQ = lle.ODD  # the queries the tie runs are counted on
MARGIN = 64
MIN_ALLOWED = 40        # the last stage searches at least NQ + MARGIN queries, and every outcome occurs
MIN_ALLOWED_FEW = 24    # the last stage searches at most NQ - MARGIN
BAND_P = (1.0, 0.3, 0.02, 0.001)
CAPS = (3, 50, 1024)
_scans = {}


class NoGpu:
    """granne_amd for lle.World on a machine without a GPU: World.a's handle holds nothing and answers World.a's two
    questions about the defaults."""

    class Granne:
        def __init__(self, *a, **kw):
            pass

        def set_option(self, option, value):
            pass

        def get_option(self, option):
            from granne_amd import _lib
            return {_lib.OPT_SEEN_MIN: NQ, _lib.OPT_SKETCH: 1}[option]

        def get_sketch(self):
            return None

        def close(self):
            pass


def band_mask(rows, seed=100):
    """One filter for all queries, as pm.density_mask: a row is allowed with probability 1.0 / 0.3 / 0.02 / 0.001 in the
    first .. fourth quartile band of rows[:, 0]."""
    c = rows[:, 0]
    q1, q2, q3 = np.quantile(c, [0.25, 0.5, 0.75])
    p = np.where(c < q1, BAND_P[0], np.where(c < q2, BAND_P[1], np.where(c < q3, BAND_P[2], BAND_P[3])))
    return np.random.default_rng(seed).random(len(c)) < p


def pf_model(world, case, nq, min_allowed, stages, fallback, k=K):
    """pm.postfiltered over the case's first nq queries under band_mask; computed once per World and argument tuple."""
    key = ("pf", case.name, nq, min_allowed, tuple(stages), fallback, k)
    if key not in world.models:
        world.models[key] = pm.postfiltered(world.orc, case.oix, case.q[:nq], band_mask(case.el), k, min_allowed, stages, fallback)
    return world.models[key]


def pending_sets(a, n_stages):
    """the queries stage s of the model searched (the fallback's codes lie above every stage)"""
    return [np.nonzero(a.stage >= s)[0] for s in range(n_stages)]


class Scan:
    """rm.full_scan of a case's first nq queries, once per session (rows and queries come from seeds: the same in every
    World), with its ids narrowed to 16 bits; called like rm.full_scan, it answers any subset of those queries."""

    def __init__(self, orc, case, nq):
        assert len(case.el) < 65536
        ids, self.ds = rm.full_scan(orc, case.el, case.q[:nq])
        self.ids = ids.astype(np.uint16)
        self.row = {case.q[i].tobytes(): i for i in range(nq)}

    def __call__(self, oracle, el, q, chunk=512):
        at = [self.row[r.tobytes()] for r in q]
        return self.ids[at].astype(np.uint64), self.ds[at]


def scan_of(orc, case, nq):
    key = (case.name, nq)
    if key not in _scans:
        _scans[key] = Scan(orc, case, nq)
    return _scans[key]


def exact_radii(orc, case, nq):
    """rm.issue_radii: the oracle's exact distance to the 3rd / 40th / 200th / 900th neighbour, -0.5, +inf, by a % 6"""
    s = scan_of(orc, case, nq)
    return rm.issue_radii({"scan": (s.ids, s.ds), "n": len(case.el)})


def radii_inside_runs(orc, case, nq):
    """how many of the finite radii are a distance the next exact neighbour shares: the cut falls inside a run of clones"""
    ds = scan_of(orc, case, nq).ds
    return sum(int(ds[a, rm.RANKS[a % 6] - 1] == ds[a, rm.RANKS[a % 6]]) for a in range(nq) if a % 6 < 4)


def walk_radii(world, case, nq, stages):
    """Radii that need no scan, from the oracle's longest walk: the distance at places 3, 80 and 200 of the last stage's
    list, one beyond that list's end (the fallback's), -0.5, +inf, by a % 6."""
    d = world.want(case, stages[-1], stages[-1])[1][:nq]
    r = np.zeros(nq, np.float32)
    for a in range(nq):
        j = a % 6
        r[a] = -0.5 if j == 4 else np.inf if j == 5 else d[a, -1] * np.float32(1.05) if j == 3 else d[a, (3, 80, 200)[j] - 1]
    return r


def rg_model(world, case, nq, radii, cap, stages, fallback):
    """rm.search_range over the case's first nq queries; computed once per World and argument tuple. The exact fallback's
    scan is the session's one where there is one for these queries."""
    key = ("rg", case.name, nq, radii.tobytes(), cap, tuple(stages), fallback)
    if key not in world.models:
        shared, own = _scans.get((case.name, nq)), rm.full_scan
        try:
            if shared is not None:
                rm.full_scan = shared
            world.models[key] = rm.search_range(world.orc, case.oix, case.q[:nq], radii, cap, stages, fallback)
        finally:
            rm.full_scan = own
    return world.models[key]


def tie_runs(case, E, S, nq=TIE_NQ):
    """how many of the first nq queries have one distance at places E - 1 .. 64 S of the oracle's list of 64 S + 1 entries:
    the key a register list of 64 S keys pushes off its end ties with the key at place max_search - 1"""
    d = case.oix.search_batch(case.q[:nq], 64 * S + 1, 64 * S + 1)[1]
    return int((d[:, E - 1] == d[:, 64 * S]).sum())


def pf_preconditions(world, case):
    """The post-filtered call's preconditions, from the model; returns the three answers (MIN_ALLOWED exact and short,
    MIN_ALLOWED_FEW exact)."""
    a = pf_model(world, case, PF_NQ, MIN_ALLOWED, STAGES, pm.EXACT)
    s = pf_model(world, case, PF_NQ, MIN_ALLOWED, STAGES, pm.SHORT)
    few = pf_model(world, case, PF_NQ, MIN_ALLOWED_FEW, STAGES, pm.EXACT)
    assert min(a.outcome_counts(3)) >= 4 and s.outcome_counts(3) == a.outcome_counts(3), (a.outcome_counts(3), s.outcome_counts(3))
    assert a.per_stage[0] == PF_NQ and a.per_stage[1] >= NQ + MARGIN and a.per_stage[2] >= NQ + MARGIN, a.per_stage
    assert few.per_stage[1] >= NQ + MARGIN and MARGIN <= few.per_stage[2] <= NQ - MARGIN, few.per_stage
    return a, s, few


def rg_preconditions(world, case, fallback, cap):
    """The range call's: every stage code occurs, stages 0 and 1 search NQ queries or more and stage 2 fewer."""
    a = rg_model(world, case, RG_NQ, exact_radii(world.orc, case, RG_NQ), cap, STAGES, fallback)
    code = rm.STAGE_EXACT if fallback == rm.EXACT else rm.STAGE_SHORT
    assert set(a.stage.tolist()) == {0, 1, 2, code}
    assert a.per_stage[0] == RG_NQ and a.per_stage[1] >= NQ and MARGIN <= a.per_stage[2] < NQ, a.per_stage
    return a


# ---- the tests -----------------------------------------------------------------------------------------------------------
_world = []


def host_world(oracle):
    if not _world:
        _world.append(lle.World(NoGpu, oracle))
    return _world[0]


def test_every_stage_has_tie_runs_across_its_lists_end(oracle):
    """A "clones": at least 16 of 2,500 queries per stage have one distance from place E - 1 to place 64 S, so every stage
    of [50, 120, 250] hands walks over; on A "uniform" and with the stages [16, 64, 256] of the entries' own tests none has."""
    w = host_world(oracle)
    clones, uniform = w.a("clones"), w.a("uniform")
    runs = [tie_runs(clones, E, S) for E, S in zip(STAGES, SLOTS)]
    print("tie runs at places E - 1 .. 64 S, of", TIE_NQ, "queries:", dict(zip(STAGES, runs)))
    assert min(runs) >= 16, runs
    assert [tie_runs(uniform, E, S) for E, S in zip(STAGES, SLOTS)] == [0, 0, 0]
    assert [tie_runs(clones, E, S) for E, S in zip([16, 64, 256], [1, 2, 8])] == [0, 0, 0]  # (runs of 49 and more: a group has 40)


def test_the_postfiltered_call_reaches_every_outcome_and_both_sides_of_the_threshold(oracle):
    w = host_world(oracle)
    a, s, few = pf_preconditions(w, w.a("clones"))
    print("post-filtered, min_allowed", MIN_ALLOWED, "per stage", a.per_stage, "outcomes", a.outcome_counts(3))
    print("post-filtered, min_allowed", MIN_ALLOWED_FEW, "per stage", few.per_stage, "outcomes", few.outcome_counts(3))
    assert a.unfinished == a.outcome_counts(3)[3] == s.unfinished
    assert (a.stage[a.stage < 3] == s.stage[s.stage < 3]).all()
    mask = band_mask(w.a("clones").el)
    for x in (a, s, few):  # what a model answers is allowed, and ascends
        live = x.ids != pm.NONE
        assert mask[x.ids[live].astype(np.int64)].all() and (live.sum(axis=1) == x.counts).all()
        assert (np.diff(x.dists, axis=1) >= 0)[live[:, 1:]].all()


def test_the_range_call_reaches_every_stage_and_cuts_inside_runs(oracle):
    w = host_world(oracle)
    case = w.a("clones")
    inside = radii_inside_runs(oracle, case, RG_NQ)
    print("finite radii that the next neighbour shares:", inside, "of", RG_NQ * 4 // 6)
    assert inside >= 64
    for fallback in (rm.EXACT, rm.SHORT):
        a = rg_preconditions(w, case, fallback, 50)
        print("range,", fallback, "per stage", a.per_stage, "answered", [int((a.stage == s).sum()) for s in range(3)], "fallback", a.unfinished)
    a3 = rg_preconditions(w, case, rm.EXACT, 3)
    assert (a3.found < 3).any() and (a3.found == 3).any() and (a3.found > 3).any()
    r = exact_radii(oracle, case, RG_NQ)
    assert (r[4::6] == -0.5).all() and np.isinf(r[5::6]).all() and (a3.found[4::6] == 0).all() and (a3.found[5::6] == len(case.el)).all()


def test_the_one_kernel_worlds_reach_the_threshold_and_every_stage(oracle):
    """A "uniform" (2,500 queries) and B (2,048): stage 0 is a launch of NQ or more, and every stage has queries to search
    under the band filter (min_allowed 24) and under the walk's radii, whose every stage code occurs."""
    w = host_world(oracle)
    for case, nq in ((w.a("uniform"), lle.ODD), (w.b(200), NQ), (w.b(96), NQ)):
        a = pf_model(w, case, nq, MIN_ALLOWED_FEW, STAGES, pm.EXACT)
        g = rg_model(w, case, nq, walk_radii(w, case, nq, STAGES), 50, STAGES, rm.SHORT)
        print(case.name, "post-filtered per stage", a.per_stage, "outcomes", a.outcome_counts(3), "range per stage", g.per_stage)
        assert a.per_stage[0] >= NQ and min(a.per_stage) >= MARGIN, (a.per_stage, a.outcome_counts(3))
        assert g.per_stage[0] >= NQ and set(g.stage.tolist()) == {0, 1, 2, rm.STAGE_SHORT}
