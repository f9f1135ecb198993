"""A CPU model of RwGranneBuilder (src/index/rw/mod.rs:15-224) under the BATCHED schedule the GPU handle uses
(TEST INFRASTRUCTURE; a plain helper module, imported by tests/test_rw_model.py and tests/test_gpu_rw_builder.py).

Written from rw/mod.rs on top of oracle.pyref.Builder's _select / _apply / _select_neighbors, which
tests/test_oracle_search.py holds against the C oracle. Per element it is GranneBuilder::index_element
(src/index/mod.rs:805-846) as rw/mod.rs:159-169 calls it: the config's num_neighbors on every layer (never halved), no
final per-row limit pass, no reinsertion. The rows an insert call puts into the current layer are indexed in sub-batches
of clamp(nodes in the layer / batch_div, 1, batch_max) members: every member searches and selects against the graph as
it stood when its sub-batch began, then the link updates are applied in id order. A sub-batch never spans a promotion.

fast=True (the default) takes the searches, select_neighbors and the distances from the C oracle -- the same functions
pyref restates, checked against each other in tests/test_rw_model.py on a whole insert sequence; fast=False is pyref
alone (pure Python: small cases only)."""
import numpy as np

from oracle import oracle, pyref

UNUSED = pyref.UNUSED


class _OracleBacked(pyref.Builder):
    """pyref.Builder whose distance evaluations run in the C oracle; the control flow stays pyref's."""

    frozen = None  # oracle.Index over previous layers + the current layer as the sub-batch found it

    def _select(self, nn, ms, prev_layers, layer, idx):  # mod.rs:812-832
        el = self.elements
        if oracle.dist(el[idx], el[idx]) > pyref.EPS100:
            return None
        # entry through the previous layers at (1, 1), or id 0, then search_for_neighbors on the current layer:
        # Granne::search over previous + current
        candidates = [(i, d) for i, d in self.frozen.search(el[idx], ms, ms) if i != idx]
        neighbors = self._select_neighbors(candidates, nn)
        if nn // 2 < len(neighbors) and neighbors[nn // 2][1] < pyref.EPS100:
            return None
        return neighbors

    def _select_neighbors(self, candidates, max_neighbors):  # mod.rs:849-883
        if len(candidates) <= max_neighbors:
            return list(candidates)
        return oracle.select_neighbors(self.elements, [c[0] for c in candidates], [c[1] for c in candidates], max_neighbors)

    def _add_and_limit_neighbors(self, node, node_id, extra, num_neighbors):  # mod.rs:923-959
        el = self.elements
        neighbors = []
        for x in node:
            if x == UNUSED:
                break
            neighbors.append(x)
        candidates = [(n, oracle.dist(el[node_id], el[n])) for n in neighbors] + list(extra)
        candidates.sort(key=lambda c: (c[1], c[0]))
        kept = self._select_neighbors(candidates, num_neighbors)
        for k in range(len(node)):
            node[k] = kept[k][0] if k < len(kept) else UNUSED


class RwModel:
    def __init__(self, builder_layers, elements, config, max_elements, fast=True):
        """RwGranneBuilder::new after builder.build() (rw/mod.rs:32-61). builder_layers: the layers of a builder built
        over `elements` with expected_num_elements = max_elements (UNUSED-padded matrices; [] for no elements).
        config: num_neighbors, max_search, layer_multiplier and optionally batch_max (65536), batch_div (8)."""
        self.nn = int(config["num_neighbors"])
        self.ms = int(config["max_search"])
        self.mult = float(config["layer_multiplier"])
        self.batch_max = int(config.get("batch_max", 65536))
        self.batch_div = int(config.get("batch_div", 8))
        self.max_elements = int(max_elements)
        self.fast = fast
        self.sub_batches = []  # members of every sub-batch indexed so far, in order
        elements = np.ascontiguousarray(elements)
        self.n = elements.shape[0]
        self.elements = np.zeros((max(self.max_elements, self.n), elements.shape[1]), elements.dtype)
        self.elements[: self.n] = elements
        layers = [np.array(l, np.uint32).reshape(-1, self.nn) for l in builder_layers]
        self.prev = layers[:-1]
        current = layers[-1] if layers else np.zeros((0, self.nn), np.uint32)  # builder.layers.pop() or an empty layer, :38-41
        assert current.shape[0] == self.n
        rows = max(current.shape[0], pyref.compute_num_elements_in_layer(self.max_elements, self.mult, len(self.prev)))
        self.current = self._resized(current, rows)  # :43-48
        cls = _OracleBacked if fast else pyref.Builder
        self._b = cls(self.elements, num_neighbors=self.nn, max_search=self.ms, layer_multiplier=self.mult,
                      reinsert_elements=False)

    @classmethod
    def new(cls, builder_layers, elements, config, max_elements, fast=True):
        return cls(builder_layers, elements, config, max_elements, fast)

    def _resized(self, layer, rows):
        out = [[int(x) for x in r] for r in layer[:rows]]
        out.extend([UNUSED] * self.nn for _ in range(rows - len(out)))
        return out

    def __len__(self):
        return self.n

    def capacity(self):
        return len(self.current)

    # rw/mod.rs:103-182
    def insert_batch(self, rows):
        rows = np.ascontiguousarray(rows, self.elements.dtype)
        ids, at = [], 0
        while at < len(rows):
            if self.n >= self.max_elements:  # :104-106
                break
            if self.n >= len(self.current):  # time to create a new layer, :118-135
                self.prev.append(np.array(self.current, np.uint32).reshape(-1, self.nn))
                rows_next = pyref.compute_num_elements_in_layer(self.max_elements, self.mult, len(self.prev))
                assert rows_next >= self.n  # :137
                self.current = self._resized(self.current, rows_next)
            take = min(len(rows) - at, len(self.current) - self.n)  # :141
            first = self.n
            self.elements[first:first + take] = rows[at:at + take]  # :146-148
            self.n += take
            self._index(first, take)
            ids.extend(range(first, first + take))  # :142
            at += take
        return ids

    def insert(self, row):
        ids = self.insert_batch(np.asarray(row).reshape(1, -1))
        return ids[0] if ids else None

    def _index(self, first, take):
        b, pos = self._b, 0
        while pos < take:
            batch = min(max(1, (first + pos) // max(1, self.batch_div)), self.batch_max, take - pos)
            members = range(first + pos, first + pos + batch)
            self.sub_batches.append(batch)
            if self.fast:
                b.frozen = oracle.Index(self.elements[: self.n], self.prev + [np.array(self.current[: self.n], np.uint32).reshape(-1, self.nn)])
            # index_element with self.config, rw/mod.rs:162: num_neighbors is not halved
            chosen = [b._select(self.nn, self.ms, self.prev, self.current, idx) for idx in members]  # the graph is frozen
            for idx, neighbors in zip(members, chosen):
                if neighbors is not None:
                    b._apply(self.current, idx, neighbors)
            pos += batch

    def layers(self):
        """Previous layers followed by the current layer's first len rows."""
        return [np.array(l, np.uint32) for l in self.prev] + [np.array(self.current[: self.n], np.uint32).reshape(-1, self.nn)]

    def index(self):
        """The live graph as an oracle.Index, or None while there is no previous layer (searches return nothing)."""
        if not self.prev:
            return None
        return oracle.Index(self.elements[: self.n].copy(), self.layers())

    # rw/mod.rs:184-207
    def search(self, q, max_search, k):
        if not self.prev:  # index.search(..).first() is None
            return []
        q = np.ascontiguousarray(q, self.elements.dtype)
        if self.fast:
            return self.index().search(q, max_search, k)
        return pyref.search(self.layers(), self.elements, q, max_search, k)
