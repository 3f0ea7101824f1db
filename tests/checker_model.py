"""The reference's linearizability checker on Python objects, dicts and lists:
operation.go, lib/graph.go (Add, Remove, AddEdge, RemoveEdge, visit, Cycle), checker.go:21-104 and
History.Linearizable (history.go:55-71).

The oracle's `oracle_linearizable` and the kernels of lin_kernel.h keep an adjacency matrix or
rows of vertex words, decide by a reach whether a merge closed a cycle, and bound the cut by the
successors' ends.  None of that is here: a vertex is an `Operation` object, the graph is the three
maps of graph.go:5-9, and every read runs Cycle() and the cut of checker.go:90-100 as written.

Where Go leaves the answer open, the project's stated choice is taken: a Go map is iterated in
insertion order of the vertices (`Graph.each`), and sort.Sort(byTime) is stable by start.  `shuffle`
replaces the first by a caller's order, to measure how far Go's own answer depends on it; the
default is insertion order.
"""


class Operation:
    """operation.go:5-11; input is None for a read, output is None for a write."""

    def __init__(self, input, output, start, end):
        self.input, self.output, self.start, self.end = input, output, start, end

    def happen_before(self, b):                            # operation.go:13-15
        return self.end < b.start

    def concurrent(self, b):                               # operation.go:17-19
        return not self.happen_before(b) and not b.happen_before(self)


class Graph:
    """lib/graph.go:5-83, 180-232.  A Set is a dict used as an insertion-ordered set."""

    def __init__(self, shuffle=None):
        self.vertices, self.frm, self.to = {}, {}, {}
        self.seq, self.n, self.shuffle = {}, 0, shuffle

    def each(self, s):
        """`for v := range set`: the vertices of `s` in the order they entered the graph."""
        vs = sorted(s, key=self.seq.__getitem__)
        return self.shuffle(vs) if self.shuffle else vs

    def has(self, v):
        return v in self.vertices

    def add(self, v):
        if not self.has(v):
            self.vertices[v] = True
            self.frm[v], self.to[v] = {}, {}
            self.seq[v], self.n = self.n, self.n + 1

    def remove(self, v):
        if not self.has(v):
            return
        del self.vertices[v]
        for u in self.vertices:
            self.frm[u].pop(v, None)
            self.to[u].pop(v, None)
        del self.frm[v], self.to[v]

    def add_edge(self, a, b):
        if a is b:
            raise RuntimeError("graph: adding self edge")
        self.add(a)
        self.add(b)
        self.frm[a][b] = True
        self.to[b][a] = True

    def remove_edge(self, a, b):
        if not self.has(a) or not self.has(b):
            return
        self.frm[a].pop(b, None)
        self.to[b].pop(a, None)

    def visit(self, v, colors):                            # graph.go:180-192, on a stack of its own
        colors[v] = "gray"
        stack = [(v, iter(self.each(self.frm[v])))]
        while stack:
            v, it = stack[-1]
            for u in it:
                if colors[u] == "gray":
                    return True
                if colors[u] == "white":
                    colors[u] = "gray"
                    stack.append((u, iter(self.each(self.frm[u]))))
                    break
            else:
                colors[v] = "black"
                stack.pop()
        return False

    def cycle(self):                                       # graph.go:212-232
        colors = {v: "white" for v in self.vertices}
        for v in self.each(self.vertices):
            if colors[v] == "white" and self.visit(v, colors):
                return [u for u, c in colors.items() if c == "gray"]
        return None


class Checker:
    """checker.go:11-104."""

    def __init__(self, shuffle=None):
        self.shuffle, self.g = shuffle, Graph(shuffle)

    def add(self, o):                                      # 21-33
        if self.g.has(o):
            return
        self.g.add(o)
        for v in self.g.each(self.g.vertices):
            if v.happen_before(o):
                self.g.add_edge(v, o)

    def match(self, read):                                 # 44-52
        for v in self.g.each(self.g.vertices):
            if read.output == v.input:
                return v
        return None

    def merge(self, read, write):                          # 55-67
        for s in self.g.each(self.g.to[read]):
            if s is not write:
                self.g.add_edge(s, write)
        if read.end < write.end:
            write.end = read.end
        self.g.remove(read)

    def linearizable(self, history):                       # 69-104
        self.g = Graph(self.shuffle)
        history = sorted(history, key=lambda o: o.start)   # stable
        anomaly = []
        for i, o in enumerate(history):
            self.add(o)
            if o.input is None:
                j = i + 1
                while j < len(history) and o.concurrent(history[j]):
                    if history[j].output is None:
                        self.add(history[j])
                    j += 1
                m = self.match(o)
                if m is not None:
                    self.merge(o, m)
                cyc = self.g.cycle()
                if cyc is not None:
                    anomaly.append(o)
                    for u in cyc:
                        for v in cyc:
                            if v in self.g.frm[u] and u.start > v.end:
                                self.g.remove_edge(u, v)
        return anomaly


def anomalies(ops, shuffle=None):
    """len(checker.linearizable) of one partition [(input, output, start, end)], None for nil."""
    return len(Checker(shuffle).linearizable([Operation(*o) for o in ops]))


def as_ops(part):
    """A partition as the histories record it, [(is_write, value, start, end)], as the worker
    hands it to the checker (benchmark.go:246-275): a write has its value as input, a read its
    value as output - 0 for a read of nil, which equals no write's input."""
    return [(v, None, s, e) if w else (None, v, s, e) for (w, v, s, e) in part]


def linearizable(shards, shuffle=None):
    """History.Linearizable (history.go:55-71): the sum over the partitions {key: [ops]}."""
    return sum(anomalies(as_ops(p), shuffle) for p in shards.values())
