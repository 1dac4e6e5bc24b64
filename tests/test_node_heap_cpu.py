"""CPU: the reference node order of the batched trees (minotaur_amd/csrc/
node_heap.h: TreeManager's bfs NodeHeap, lazy pruning, node ids, pool slots)
against a plain restatement, through tests/node_heap_main.cpp built with the
host compiler and -fsanitize=address,undefined.

The restatement scans for the best node as oracle/glob_tree.py's _Heap does.
Bounds lie on a grid spaced 1e-3 (many exact ties: depth and id decide) plus a
few pairs 5e-7 apart, each pair at least 1e-3 from every other value: within
the comparator's 1e-6 band the pair ties too, and the comparator stays a
strict weak order on these inputs, so the scan and std::pop_heap must agree.
Slot numbers are free to differ between policies; what is checked is that a
slot handed out is never the slot of a node still open, and that the high-water
mark rises only when no slot is free."""
import math
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
MAIN = os.path.join(ROOT, 'tests', 'node_heap_main.cpp')
INC = os.path.join(ROOT, 'minotaur_amd', 'csrc')
CXX = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')

GRID = [k * 1e-3 for k in range(31)]
PAIRS = [(-0.005, -0.005 + 5e-7), (0.035, 0.035 + 5e-7), (0.040, 0.040 + 5e-7)]
VALUES = GRID + [v for p in PAIRS for v in p]
INF = math.inf


def should_prune(lb, inc):
    return lb > inc - 1e-6 or abs(inc - lb) / (abs(inc) + 1e-6) * 100.0 < 1e-6


def better(a, b):
    """a leaves the heap before b (NodeHeap.cpp:24-47)."""
    if a['lb'] > b['lb'] + 1e-6:
        return False
    if a['lb'] < b['lb'] - 1e-6:
        return True
    if a['depth'] != b['depth']:
        return a['depth'] < b['depth']
    return a['id'] > b['id']


class Model:
    """The order, the ids and the slot count; never a slot number."""

    def __init__(self, cap):
        self.heap = [dict(lb=-INF, depth=0, id=0)]
        self.front = []
        self.next_id, self.hw, self.nfree, self.cap = 1, 1, 0, cap

    def take(self, batch, inc):
        nodes, self.front = self.front[:batch], self.front[batch:]
        pruned = []
        while len(nodes) < batch and self.heap:
            best = 0
            for i in range(1, len(self.heap)):
                if better(self.heap[i], self.heap[best]):
                    best = i
            top = self.heap.pop(best)
            (pruned if should_prune(top['lb'], inc) else nodes).append(top)
        self.nfree += len(pruned)
        fits = self.hw + max(0, len(nodes) - self.nfree) <= self.cap
        self.nfree += len(nodes)
        return nodes, pruned, fits

    def slot(self):
        """None: any free slot below the high-water mark; else the new slot."""
        if self.nfree > 0:
            self.nfree -= 1
            return None
        self.hw += 1
        return self.hw - 1

    def kids(self, node, lb):
        out = []
        for _ in range(2):
            out.append((self.next_id, self.slot()))
            self.heap.append(dict(lb=lb, depth=node['depth'] + 1, id=self.next_id))
            self.next_id += 1
        return out

    def requeue(self, node):
        self.front.append(node)
        return [(node['id'], self.slot())]

    def open_ids(self):
        return [n['id'] for n in self.heap + self.front]


class Script:
    """The commands for node_heap_main and, line for line, what the
    restatement expects back."""

    def __init__(self):
        self.lines, self.expect, self.m, self.round = [], [], None, []

    def reset(self, cap):
        self.m = Model(cap)
        self.lines.append(f'reset {cap}')
        self.expect.append(('reset', cap))

    def take(self, batch, inc):
        nodes, pruned, fits = self.m.take(batch, inc)
        self.round = nodes
        self.lines.append(f'take {batch} {float(inc).hex()}')
        self.expect.append(('take', [n['id'] for n in nodes], [n['id'] for n in pruned], fits,
                            self.m.hw))
        return nodes, pruned, fits

    def kids(self, i, lb):
        self.lines.append(f'kids {i} {float(lb).hex()}')
        self.expect.append(('slots', self.m.kids(self.round[i], lb), self.m.open_ids()))

    def requeue(self, i):
        self.lines.append(f'requeue {i}')
        self.expect.append(('slots', self.m.requeue(self.round[i]), self.m.open_ids()))

    def end(self):
        self.lines.append('end')
        self.expect.append(('state', len(self.m.open_ids()), self.m.hw))


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    if CXX is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path_factory.mktemp('node_heap') / 'node_heap_main')
    subprocess.run([CXX, '-std=c++17', '-O1', '-g', '-Wall', '-Werror',
                    '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', INC, MAIN,
                    '-o', exe], check=True)
    return exe


def check(prog, sc):
    r = subprocess.run([prog], input='\n'.join(sc.lines) + '\n', capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr[-3000:]
    out = iter(r.stdout.splitlines())
    slot_of, cap = {}, 0
    for e in sc.expect:
        if e[0] == 'reset':
            slot_of, cap = {0: 0}, e[1]
            continue
        got = next(out).split()
        if e[0] == 'take':
            _, ids, pruned, fits, hw = e
            assert got[0] == 'take' and int(got[1]) == len(pruned), (got, e)
            assert int(got[2]) == int(fits), (got, e, hw)
            pairs = [tuple(map(int, t.split(':'))) for t in got[4:]]
            assert int(got[3]) == len(pairs)
            assert [p[0] for p in pairs] == ids, (got, e)            # the popped ids in order
            for i, sl in pairs:
                assert slot_of.pop(i) == sl, 'a node came back from another slot'
            for i in pruned:
                del slot_of[i]
        elif e[0] == 'slots':
            _, handed, open_ids = e
            assert got[0] == 'slots' and len(got) == 1 + len(handed)
            for (i, new), sl in zip(handed, map(int, got[1:])):
                assert 0 <= sl < cap
                assert sl not in slot_of.values(), f'slot {sl} still holds an open node'
                if new is not None:
                    assert sl == new, 'a new slot is the high-water mark'
                slot_of[i] = sl
            assert sorted(slot_of) == sorted(open_ids)
        else:
            assert got == ['state', str(e[1]), str(e[2])], (got, e)   # open(), high-water mark
    assert next(out, None) is None


def seeded(seed, cap, rounds=300):
    """Rounds over several trees: a tree ends when it is empty or its pool
    is refused, then the next one starts."""
    rng = random.Random(seed)
    sc = Script()
    seen = dict(cut_short=0, wide=0, refused=0, front_first=0, pair=0, trees=0)
    inc = INF
    for _ in range(rounds):
        if sc.m is None or not sc.m.open_ids():
            sc.reset(cap)
            inc = INF
            seen['trees'] += 1
        if rng.random() < 0.08:   # a better incumbent, on, next to and between the bounds
            v = rng.choice(VALUES[8:]) + rng.choice([0.0, 1e-6, 2e-6, 5e-7, -5e-7, 5e-4])
            inc = min(inc, v)
        batch = rng.choice([1, 1, 2, 3, 4, 8, 64])
        n_open = len(sc.m.open_ids())
        heap_best = min((n['lb'] for n in sc.m.heap), default=INF)
        front = [n['lb'] for n in sc.m.front[:batch]]
        nodes, pruned, fits = sc.take(batch, inc)
        seen['cut_short'] += bool(pruned) and len(nodes) < min(batch, n_open)
        seen['wide'] += batch > n_open
        seen['front_first'] += any(lb > heap_best + 1e-3 for lb in front)
        seen['pair'] += any(0 < abs(a['lb'] - b['lb']) < 1e-6 for a, b in zip(nodes, nodes[1:]))
        if not fits:
            seen['refused'] += 1
            sc.m = None
            continue
        for i in range(len(nodes)):   # (the tree hovers around 30 open nodes)
            what = rng.random()
            if what < (0.75 if len(sc.m.open_ids()) < 30 else 0.4):
                sc.kids(i, rng.choice(VALUES))
            elif what > 0.9:
                sc.requeue(i)
        sc.end()
    return sc, seen


@pytest.mark.parametrize('seed,cap', [(1, 100000), (2, 100000), (3, 100000), (4, 24), (5, 40)])
def test_seeded_rounds(prog, seed, cap):
    sc, seen = seeded(seed, cap)
    print(seed, cap, seen)
    check(prog, sc)
    assert seen['cut_short'] and seen['wide'] and seen['front_first'] and seen['trees'] > 1
    assert seen['pair']
    assert (seen['refused'] > 0) == (cap < 1000)


def test_named_cases(prog):
    sc = Script()
    # incumbent +inf prunes nothing, the root's -inf bound included; a batch
    # wider than the tree takes what is open
    sc.reset(100)
    nodes, pruned, fits = sc.take(64, INF)
    assert [n['id'] for n in nodes] == [0] and not pruned and fits
    sc.kids(0, 0.010)
    sc.end()
    nodes, _, _ = sc.take(64, INF)
    assert [n['id'] for n in nodes] == [2, 1]          # equal bound and depth: the larger id
    sc.kids(0, 0.020)
    sc.kids(1, 0.005)
    sc.end()
    # a requeued node keeps its id and runs ahead of a better heap top
    nodes, _, _ = sc.take(3, INF)
    assert [n['id'] for n in nodes] == [6, 5, 4] and nodes[2]['lb'] == 0.020
    sc.kids(0, 0.001)
    sc.requeue(2)
    sc.end()
    nodes, _, _ = sc.take(2, INF)
    assert [(n['id'], n['lb']) for n in nodes] == [(4, 0.020), (8, 0.001)]
    sc.kids(0, 0.030)
    sc.kids(1, 0.030)
    sc.end()
    # a round cut short by pruning: under incumbent 0.020 + 5e-7 the node at
    # 0.020 (inside the 1e-6 band) and the four at 0.030 go, one node runs
    nodes, pruned, _ = sc.take(4, 0.020 + 5e-7)
    assert [n['id'] for n in nodes] == [7] and len(pruned) == 5
    sc.end()
    # the 1e-6 band: two bounds 5e-7 apart tie, so depth and id decide
    sc.reset(100)
    sc.take(1, INF)
    sc.kids(0, 0.035 + 5e-7)
    sc.end()
    sc.take(1, INF)
    sc.kids(0, 0.035)
    sc.end()
    nodes, _, _ = sc.take(3, INF)
    assert [n['id'] for n in nodes] == [1, 4, 3]        # the shallower 0.035 + 5e-7 first
    sc.end()
    # a pool that fills exactly: 3 slots hold 3 open nodes, and the round that
    # may need a fourth is refused before it runs
    sc.reset(3)
    assert sc.take(1, INF)[2]
    sc.kids(0, 0.001)
    sc.end()
    assert sc.take(1, INF)[2]
    sc.kids(0, 0.002)
    sc.end()
    assert sc.m.hw == 3 and len(sc.m.open_ids()) == 3
    assert not sc.take(1, INF)[2]
    # ... and at two nodes a round: high-water mark 2, two nodes, no free slot
    sc.reset(3)
    sc.take(1, INF)
    sc.kids(0, 0.001)
    sc.end()
    assert sc.m.hw == 2 and not sc.take(2, INF)[2]
    # a pruned node's slot counts as free: at high-water mark 3 of 4 slots two
    # nodes alone do not fit, the same two after a pruned third do
    for batch, n_pruned, ok in ((2, 0, False), (3, 1, True)):
        sc.reset(4)
        sc.take(1, INF)
        sc.kids(0, 0.009)
        sc.end()
        sc.take(1, INF)
        sc.kids(0, 0.001)
        sc.end()
        nodes, pruned, fits = sc.take(batch, 0.005)
        assert sc.m.hw == 3 and len(nodes) == 2 and len(pruned) == n_pruned and fits == ok
    check(prog, sc)
