// Reference node order (mgpu_bnb_config / mgpu_glob_config order 2), kept on
// the host for the batched linear tree (bnb.cpp) and the batched spatial tree
// (glob_runtime.cpp): TreeManager's "bfs" NodeHeap with the reference's
// comparator valueGreaterThan (NodeHeap.cpp:24-47: bound within 1e-6,
// tie-break score (0 in BranchAndBound), shallower first, then the larger
// node id on top) and the same std::push_heap / std::pop_heap, node ids
// assigned as TreeManager does (root 0, children in branch order,
// TreeManager.cpp:97-136, 232-249), open nodes pruned lazily at the top by
// the incumbent (TreeManager::getCandidate, :162-186), pool slots recycled.
// Standard library only: tests/node_heap_main.cpp compiles it on its own.
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

class NodeHeap {
 public:
  struct Node {
    double lb;
    int depth;
    long long id;
    int slot;
  };
  struct Round {
    std::vector<Node> nodes;   // the round's nodes in pop order
    int pruned = 0;            // open nodes the incumbent pruned on the way
    bool fits = true;          // the pool holds the round's children at worst
  };

  // TreeManager::shouldPrune_ (:403-413) with solAbs_tol / solRel_tol 1e-6
  static bool should_prune(double lb, double inc) {
    return lb > inc - 1e-6 || std::fabs(inc - lb) / (std::fabs(inc) + 1e-6) * 100.0 < 1e-6;
  }

  // the root is node 0 in slot 0 with no bound yet
  void reset(int capacity) {
    heap_.assign(1, Node{-INFINITY, 0, 0, 0});
    front_.clear();
    free_.clear();
    next_id_ = 1;
    hw_ = 1;
    cap_ = capacity;
  }

  // Up to `batch` nodes: the requeued ones first, in order (their process()
  // call goes on), then TreeManager::getCandidate: the heap top, pruned lazily
  // under `inc`, then removed.  Two children per node, in the round's own
  // slots, the free ones, then new ones, must fit the pool.  The round's slots
  // are free from here on: every caller reads a popped node's data from the
  // gathered batch buffers (the spatial tree's per-slot branching records are
  // copied out at the start of its lockstep), never from its pool slot, so a
  // child may be written there.
  Round take(int batch, double inc) {
    Round r;
    size_t nf = 0;
    for (; nf < front_.size() && (int)r.nodes.size() < batch; ++nf) r.nodes.push_back(front_[nf]);
    front_.erase(front_.begin(), front_.begin() + (long)nf);
    while ((int)r.nodes.size() < batch && !heap_.empty()) {
      std::pop_heap(heap_.begin(), heap_.end(), greater);
      const Node top = heap_.back();
      heap_.pop_back();
      if (should_prune(top.lb, inc)) {
        free_.push_back(top.slot);
        r.pruned += 1;
      } else {
        r.nodes.push_back(top);
      }
    }
    const long need = (long)r.nodes.size() - (long)free_.size();
    r.fits = hw_ + (need > 0 ? need : 0) <= cap_;
    for (const Node &n : r.nodes) free_.push_back(n.slot);
    return r;
  }

  // a pool slot for a child (or a requeued node) of the round just taken:
  // never the slot of an open node, and a new slot only when none is free
  int take_slot() {
    if (free_.empty()) return hw_++;
    const int slot = free_.back();
    free_.pop_back();
    return slot;
  }

  // a child enters with the next node id
  void push(double lb, int depth, int slot) {
    heap_.push_back(Node{lb, depth, next_id_++, slot});
    std::push_heap(heap_.begin(), heap_.end(), greater);
  }

  // a node modified by the brancher: the same node (its id) is solved again
  // right away with the bound change (PCBProcessor.cpp:295-310), ahead of the
  // heap, from the slot its record names
  void requeue(const Node &n) { front_.push_back(n); }

  int open() const { return (int)(heap_.size() + front_.size()); }
  int hw() const { return hw_; }   // pool high-water mark

  // ---- migration between ranks (MpiBranchAndBound::LoadBalance_, :78-195:
  // mgpu_glob_pick / _export_dev / _import_dev / _shard) ----------------------
  // LoadBalance_'s pop of the next S candidates (:93-105): getCandidate S
  // times as take() does it, pruned nodes freed and counted, but the nodes
  // that come out KEEP their pool slots: each one goes back under its own id
  // (put_back) or leaves for another rank (drop).  Until then they are not
  // counted in open().  Requeued nodes are mid-process and stay.
  Round hold(int S, double inc) {
    Round r;
    while ((int)r.nodes.size() < S && !heap_.empty()) {
      std::pop_heap(heap_.begin(), heap_.end(), greater);
      const Node top = heap_.back();
      heap_.pop_back();
      if (should_prune(top.lb, inc)) {
        free_.push_back(top.slot);
        r.pruned += 1;
      } else {
        r.nodes.push_back(top);
      }
    }
    return r;
  }

  // a held node that stays: the same node (bound, depth, id, slot) is open again
  void put_back(const Node &n) {
    heap_.push_back(n);
    std::push_heap(heap_.begin(), heap_.end(), greater);
  }

  // a held node that left: its slot is free
  void drop(const Node &n) { free_.push_back(n.slot); }

  // pool slots an import can still take (free ones, then new ones)
  int spare() const { return cap_ - hw_ + (int)free_.size(); }

  // MpiBranchAndBound's round-robin deal of the shared first rounds'
  // open nodes (:142-188): of the open nodes in ascending id order, the ones
  // at positions = rank (mod world) stay, with their ids and slots; the
  // others leave the heap and their slots become free.  Returns the kept count.
  int shard(int rank, int world) {
    std::vector<long long> ids;
    for (const Node &n : heap_) ids.push_back(n.id);
    std::sort(ids.begin(), ids.end());
    std::vector<Node> keep;
    for (const Node &n : heap_) {
      const long pos = (long)(std::lower_bound(ids.begin(), ids.end(), n.id) - ids.begin());
      if (pos % world == rank) keep.push_back(n);
      else free_.push_back(n.slot);
    }
    heap_.swap(keep);
    std::make_heap(heap_.begin(), heap_.end(), greater);
    return (int)heap_.size();
  }

 private:
  static bool greater(const Node &a, const Node &b) {
    if (a.lb > b.lb + 1e-6) return true;
    if (a.lb < b.lb - 1e-6) return false;
    if (a.depth < b.depth) return false;
    if (a.depth > b.depth) return true;
    return a.id < b.id;
  }
  std::vector<Node> heap_, front_;
  std::vector<int> free_;
  long long next_id_ = 1;
  int hw_ = 0, cap_ = 0;
};

// The branch order of a node's two children: QuadHandler::getBranches goes
// down then up (QuadHandler.cpp:422-471); IntVarHandler::getBranches takes
// the candidate's preferred direction first, or -- guided dive, with an
// incumbent -- down first when the incumbent's value of the variable is below
// the node's (IntVarHandler.cpp:125-190).
inline bool down_first(bool is_int, bool prefers_up, bool guided, double inc, double best_x_j,
                       double value) {
  if (!is_int) return true;
  if (guided && std::isfinite(inc) && !std::isnan(best_x_j)) return best_x_j < value;
  return !prefers_up;
}
