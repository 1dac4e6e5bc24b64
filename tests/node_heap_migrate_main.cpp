// Drives the migration methods of minotaur_amd/csrc/node_heap.h (hold,
// put_back, drop, spare, shard) from a script on stdin, one command per line,
// for tests/test_node_heap_migrate_cpu.py:
//   reset CAP     a new tree with a pool of CAP slots
//   take B INC    a round of up to B nodes under incumbent INC
//                 -> "take PRUNED N id:slot ..."
//   kids I V      both children of the round's node I, with bound V
//                 -> "slots A B"
//   hold S INC    the next S candidates, their slots kept
//                 -> "hold PRUNED N id:slot ..."
//   settle MASK   one character per held node: 1 it left (drop), 0 it stays
//                 (put_back)                        -> "state OPEN HIGHWATER SPARE"
//   import V D    a node from another rank: a slot and the next id
//                 -> "slots A"
//   shard R W     keep the open nodes at positions R (mod W) in id order
//                 -> "shard KEPT"
//   end           -> "state OPEN HIGHWATER SPARE"
// Numbers are what strtod reads (hex floats, inf).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "node_heap.h"

int main() {
  NodeHeap h;
  NodeHeap::Round r, held;
  std::string cmd, num;
  auto show = [](const char *what, const NodeHeap::Round &q) {
    std::printf("%s %d %zu", what, q.pruned, q.nodes.size());
    for (const NodeHeap::Node &n : q.nodes) std::printf(" %lld:%d", n.id, n.slot);
    std::printf("\n");
  };
  while (std::cin >> cmd) {
    if (cmd == "reset") {
      int cap;
      std::cin >> cap;
      h.reset(cap);
      held = NodeHeap::Round();
    } else if (cmd == "take") {
      int batch;
      std::cin >> batch >> num;
      r = h.take(batch, std::strtod(num.c_str(), nullptr));
      show("take", r);
    } else if (cmd == "kids") {
      size_t i;
      std::cin >> i >> num;
      const double v = std::strtod(num.c_str(), nullptr);
      const int a = h.take_slot(), b = h.take_slot();
      h.push(v, r.nodes.at(i).depth + 1, a);
      h.push(v, r.nodes.at(i).depth + 1, b);
      std::printf("slots %d %d\n", a, b);
    } else if (cmd == "hold") {
      int S;
      std::cin >> S >> num;
      held = h.hold(S, std::strtod(num.c_str(), nullptr));
      show("hold", held);
    } else if (cmd == "settle") {
      std::string mask;
      std::cin >> mask;
      if (mask == "-") mask.clear();   // no node was held
      if (mask.size() != held.nodes.size()) {
        std::fprintf(stderr, "settle: %zu marks for %zu held nodes\n", mask.size(),
                     held.nodes.size());
        return 2;
      }
      for (size_t i = 0; i < mask.size(); ++i) {
        if (mask[i] == '1') h.drop(held.nodes[i]);
        else h.put_back(held.nodes[i]);
      }
      held = NodeHeap::Round();
      std::printf("state %d %d %d\n", h.open(), h.hw(), h.spare());
    } else if (cmd == "import") {
      int depth;
      std::cin >> num >> depth;
      const int a = h.take_slot();
      h.push(std::strtod(num.c_str(), nullptr), depth, a);
      std::printf("slots %d\n", a);
    } else if (cmd == "shard") {
      int rank, world;
      std::cin >> rank >> world;
      std::printf("shard %d\n", h.shard(rank, world));
    } else if (cmd == "end") {
      std::printf("state %d %d %d\n", h.open(), h.hw(), h.spare());
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
