"""A CPU model of RwGranneBuilder with removals (TEST INFRASTRUCTURE; a plain helper module, imported by
tests/test_rw_remove_model.py and tests/test_gpu_rw_remove.py): tests/rw_model.py's RwModel, a set of removed ids, and
the live search as tests/filter_model.py's walk under `alive` over the model's layers.

What it states (include/granne_hip.h, "removing elements"): inserts never look at the removed set --
`insert_batch` IS RwModel's --, a removed element stays in the graph and is traversed, and a search returns the nearest
ALIVE elements the filtered walk finds. With nothing removed the search is RwModel.search (the reference's)."""
import numpy as np

from tests import filter_model as fm
from tests.rw_model import RwModel


class RwRemoveModel:
    def __init__(self, model):
        self.m = model  # an RwModel
        self.removed = set()

    @classmethod
    def new(cls, builder_layers, elements, config, max_elements, fast=True):
        return cls(RwModel.new(builder_layers, elements, config, max_elements, fast))

    def __len__(self):
        return len(self.m)

    def insert_batch(self, rows):
        return self.m.insert_batch(rows)

    def insert(self, row):
        return self.m.insert(row)

    def layers(self):
        return self.m.layers()

    def _mark(self, ids, remove):
        """(changed, in that state already -- a repeat within `ids` included --, ids >= len)"""
        changed = same = bad = 0
        for i in (int(x) for x in ids):
            if i >= len(self.m):
                bad += 1
            elif (i in self.removed) == remove:
                same += 1
            else:
                changed += 1
                (self.removed.add if remove else self.removed.discard)(i)
        return changed, same, bad

    def remove(self, ids):
        return self._mark(ids, True)

    def restore(self, ids):
        return self._mark(ids, False)

    def removed_count(self):
        return len(self.removed)

    def alive(self):
        a = np.ones(len(self.m), bool)
        a[sorted(self.removed)] = False
        return a

    def search(self, q, max_search, k, dist_row=None, cache=None, stats=False):
        """[(id, dist)] -- with stats=True also (n_dist, n_expand, n_adj). Without a previous layer: nothing."""
        if not self.m.prev:  # index.search(..).first() is None (rw/mod.rs:198-206)
            return ([], (0, 0, 0)) if stats else []
        if not self.removed and not stats:
            return self.m.search(q, max_search, k)  # the path the handle takes with nothing removed
        q = np.ascontiguousarray(q, self.m.elements.dtype)
        r = fm.search_filtered(self.m.layers(), self.m.elements[: len(self.m)], q, self.alive(), max_search, k, 0, dist_row, cache)
        pairs = list(zip(r.ids, [float(d) for d in r.dists]))
        c = r.counters
        return (pairs, (c["n_dist"], c["n_expand"], c["n_adj"])) if stats else pairs
