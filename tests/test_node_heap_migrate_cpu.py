"""CPU: the migration methods of the reference node order (minotaur_amd/csrc/
node_heap.h: hold, put_back, drop, spare, shard -- what mgpu_glob_pick /
_export_dev / _import_dev / _shard do on the host) against a plain
restatement, through tests/node_heap_migrate_main.cpp built with the host
compiler, once plain and once with -fsanitize=address,undefined, each run as
its own process.

The restatement scans for the best node as oracle/glob_tree.py's _Heap does.
Bounds lie on a grid spaced 1e-3, so two bounds are equal or more than 1e-6
apart and the comparator is a strict weak order: the scan and std::pop_heap
must agree whatever shape the heap array has, which is what lets a heap that
was held and put back be compared with one that never was."""
import math
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
MAIN = os.path.join(ROOT, 'tests', 'node_heap_migrate_main.cpp')
INC = os.path.join(ROOT, 'minotaur_amd', 'csrc')
CXX = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
INF = math.inf
GRID = [k * 1e-3 for k in range(40)]


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
    """The order, the ids and the slot counts; never a slot number."""

    def __init__(self, cap):
        self.heap = [dict(lb=-INF, depth=0, id=0)]
        self.next_id, self.hw, self.nfree, self.cap = 1, 1, 0, cap
        self.held = []

    def _pop(self, n, inc):
        nodes, pruned = [], []
        while len(nodes) < n and self.heap:
            best = 0
            for i in range(1, len(self.heap)):
                if better(self.heap[i], self.heap[best]):
                    best = i
            top = self.heap.pop(best)
            (pruned if should_prune(top['lb'], inc) else nodes).append(top)
        self.nfree += len(pruned)
        return nodes, pruned

    def take(self, batch, inc):
        nodes, pruned = self._pop(batch, inc)
        self.nfree += len(nodes)
        return nodes, pruned

    def hold(self, S, inc):
        self.held, pruned = self._pop(S, inc)
        return self.held, pruned

    def settle(self, mask):
        for n, gone in zip(self.held, mask):
            if gone == '1':
                self.nfree += 1
            else:
                self.heap.append(n)
        self.held = []

    def slot(self):
        if self.nfree > 0:
            self.nfree -= 1
            return None
        self.hw += 1
        return self.hw - 1

    def push(self, lb, depth):
        new = self.slot()
        self.heap.append(dict(lb=lb, depth=depth, id=self.next_id))
        self.next_id += 1
        return self.next_id - 1, new

    def shard(self, rank, world):
        ids = sorted(n['id'] for n in self.heap)
        keep = {i for p, i in enumerate(ids) if p % world == rank}
        self.nfree += len(ids) - len(keep)
        self.heap = [n for n in self.heap if n['id'] in keep]
        return sorted(keep)

    def open_ids(self):
        return sorted(n['id'] for n in self.heap)

    def spare(self):
        return self.cap - self.hw + self.nfree


class Script:
    def __init__(self, cap):
        self.m = Model(cap)
        self.cap = cap
        self.lines, self.expect, self.round = [f'reset {cap}'], [], []

    def take(self, batch, inc=INF):
        nodes, pruned = self.m.take(batch, inc)
        self.round = nodes
        self.lines.append(f'take {batch} {float(inc).hex()}')
        self.expect.append(('pop', 'take', [n['id'] for n in nodes], [n['id'] for n in pruned],
                            True))
        return nodes

    def hold(self, S, inc=INF):
        nodes, pruned = self.m.hold(S, inc)
        self.lines.append(f'hold {S} {float(inc).hex()}')
        self.expect.append(('pop', 'hold', [n['id'] for n in nodes], [n['id'] for n in pruned],
                            False))
        return nodes, pruned

    def kids(self, i, lb):
        d = self.round[i]['depth'] + 1
        handed = [self.m.push(lb, d), self.m.push(lb, d)]
        self.lines.append(f'kids {i} {float(lb).hex()}')
        self.expect.append(('slots', handed))

    def settle(self, mask):
        gone = [n['id'] for n, g in zip(self.m.held, mask) if g == '1']
        self.m.settle(mask)
        self.lines.append(f"settle {mask or '-'}")
        self.expect.append(('state', gone, len(self.m.heap), self.m.hw, self.m.spare()))

    def imp(self, lb, depth):
        self.lines.append(f'import {float(lb).hex()} {depth}')
        self.expect.append(('slots', [self.m.push(lb, depth)]))

    def shard(self, rank, world):
        before = self.m.open_ids()
        keep = self.m.shard(rank, world)
        self.lines.append(f'shard {rank} {world}')
        self.expect.append(('shard', keep, [i for i in before if i not in keep]))
        return keep

    def end(self):
        self.lines.append('end')
        self.expect.append(('state', [], len(self.m.heap), self.m.hw, self.m.spare()))

    def drain(self, batch=1, inc=INF):
        """Pops to the end, no children: the whole remaining order."""
        out = []
        while self.m.heap:
            out += [n['id'] for n in self.take(batch, inc)]
        return out


@pytest.fixture(scope='module', params=['plain', 'sanitized'])
def prog(request, tmp_path_factory):
    if CXX is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path_factory.mktemp('node_heap_migrate') / ('main_' + request.param))
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'] \
        if request.param == 'sanitized' else []
    subprocess.run([CXX, '-std=c++17', '-O1', '-g', '-Wall', '-Werror'] + flags +
                   ['-I', INC, MAIN, '-o', exe], check=True)
    return exe


def check(prog, sc):
    r = subprocess.run([prog], input='\n'.join(sc.lines) + '\n', capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr[-3000:]
    out = iter(r.stdout.splitlines())
    slot_of = {0: 0}       # open or held node id -> its pool slot
    held = {}
    for e in sc.expect:
        got = next(out).split()
        if e[0] == 'pop':
            _, what, ids, pruned, frees = e
            assert got[0] == what and int(got[1]) == len(pruned), (got, e)
            pairs = [tuple(map(int, t.split(':'))) for t in got[3:]]
            assert int(got[2]) == len(pairs)
            assert [p[0] for p in pairs] == ids, (got, e)          # the ids in pop order
            for i, sl in pairs:
                assert slot_of[i] == sl, 'a node came back from another slot'
                if frees:
                    del slot_of[i]
                else:
                    held[i] = sl
            for i in pruned:
                del slot_of[i]
        elif e[0] == 'slots':
            assert got[0] == 'slots' and len(got) == 1 + len(e[1])
            for (i, new), sl in zip(e[1], map(int, got[1:])):
                assert 0 <= sl < sc.cap
                assert sl not in slot_of.values(), f'slot {sl} still holds an open or held node'
                if new is not None:
                    assert sl == new, 'a new slot is the high-water mark'
                slot_of[i] = sl
        elif e[0] == 'shard':
            assert got == ['shard', str(len(e[1]))], (got, e)
            for i in e[2]:
                del slot_of[i]
        else:
            _, gone, n_open, hw, spare = e
            assert got == ['state', str(n_open), str(hw), str(spare)], (got, e)
            for i in gone:
                del slot_of[i]
            held.clear()
    assert next(out, None) is None


def grow(sc, rng, rounds, target=30):
    """Rounds with children until the tree holds about ``target`` open nodes."""
    for _ in range(rounds):
        if not sc.m.heap:
            break
        nodes = sc.take(rng.choice([1, 2, 3, 4]))
        for i in range(len(nodes)):
            n = len(sc.m.heap)
            if n < 4 or rng.random() < (0.85 if n < target else 0.3):
                sc.kids(i, rng.choice(GRID))
        sc.end()


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_hold_and_put_back_keeps_the_order(prog, seed):
    """hold S then put everything back, several times and at several S, in
    between rounds: every later pop comes out as from the restatement, whose
    list a hold followed by a put-back leaves as it was."""
    rng = random.Random(seed)
    sc = Script(100000)
    for _ in range(6):
        grow(sc, rng, 12)
        S = rng.choice([1, 3, 8, 50, 1000])
        nodes, pruned = sc.hold(S)
        assert not pruned and len(nodes) == min(S, len(nodes) + len(sc.m.heap))
        sc.settle('0' * len(nodes))
    assert len(sc.m.heap) > 10
    untouched = sorted(sc.m.heap, key=lambda n: n['id'])
    order = sc.drain()
    # the same order from a list that never saw a hold: the scan alone
    m2 = Model(1)
    m2.heap = [dict(n) for n in untouched]
    assert order == [n['id'] for n in m2._pop(10**9, INF)[0]]
    check(prog, sc)


def test_hold_prunes_lazily_and_dropped_slots_are_reused(prog):
    sc = Script(64)
    rng = random.Random(7)
    grow(sc, rng, 30, target=20)
    n_open, hw = len(sc.m.heap), sc.m.hw
    assert n_open >= 12
    lbs = sorted(n['lb'] for n in sc.m.heap)
    inc = lbs[8] + 5e-4                        # prunes the worst nodes once the pop reaches them
    nodes, pruned = sc.hold(1000, inc)
    assert pruned and nodes and len(nodes) + len(pruned) == n_open
    free0 = sc.m.nfree
    mask = ''.join('1' if t % 2 == 0 else '0' for t in range(len(nodes)))
    sc.settle(mask)
    assert sc.m.nfree == free0 + mask.count('1') and sc.m.hw == hw
    # imports take the freed slots before any new one
    for t in range(sc.m.nfree):
        sc.imp(GRID[t % len(GRID)], 3)
    assert sc.m.hw == hw and sc.m.nfree == 0
    sc.imp(0.002, 1)
    assert sc.m.hw == hw + 1
    sc.end()
    sc.drain(batch=3)
    check(prog, sc)


def test_hold_on_a_short_or_empty_heap(prog):
    sc = Script(8)
    nodes, pruned = sc.hold(4)
    assert [n['id'] for n in nodes] == [0] and not pruned       # the root, bound -inf
    sc.settle('0')
    sc.take(1)
    sc.end()
    nodes, pruned = sc.hold(4)
    assert not nodes and not pruned
    sc.settle('')
    sc.imp(0.5, 2)
    sc.imp(0.25, 5)
    nodes, _ = sc.hold(1)
    assert [n['id'] for n in nodes] == [2]
    sc.settle('1')
    assert sc.drain() == [1]
    check(prog, sc)


@pytest.mark.parametrize('world', [1, 2, 3, 5])
def test_shard_keeps_the_positions_of_its_rank(prog, world):
    for rank in range(world):
        rng = random.Random(11)
        sc = Script(1000)
        grow(sc, rng, 25)
        ids = sc.m.open_ids()
        assert len(ids) > 2 * world
        keep = sc.shard(rank, world)
        assert keep == ids[rank::world]
        sc.end()
        assert sc.m.spare() == 1000 - sc.m.hw + sc.m.nfree
        sc.imp(0.0155, 4)                       # a migrated node joins the kept ones
        got = sc.drain(batch=2)
        assert sorted(got) == sorted(keep + [sc.m.next_id - 1])
        check(prog, sc)
