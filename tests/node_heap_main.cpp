// Drives minotaur_amd/csrc/node_heap.h from a script on stdin, one command
// per line, for tests/test_node_heap_cpu.py:
//   reset CAP     a new tree with a pool of CAP slots
//   take B INC    a round of up to B nodes under incumbent INC
//                 -> "take PRUNED FITS N id:slot ..."
//   kids I V      both children of the round's node I, with bound V
//                 -> "slots A B"
//   requeue I     the round's node I again, ahead of the heap  -> "slots A"
//   end           the round is over                 -> "state OPEN HIGHWATER"
// Numbers are what strtod reads (hex floats, inf).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "node_heap.h"

int main() {
  NodeHeap h;
  NodeHeap::Round r;
  std::string cmd, num;
  while (std::cin >> cmd) {
    if (cmd == "reset") {
      int cap;
      std::cin >> cap;
      h.reset(cap);
    } else if (cmd == "take") {
      int batch;
      std::cin >> batch >> num;
      r = h.take(batch, std::strtod(num.c_str(), nullptr));
      std::printf("take %d %d %zu", r.pruned, r.fits ? 1 : 0, r.nodes.size());
      for (const NodeHeap::Node &n : r.nodes) std::printf(" %lld:%d", n.id, n.slot);
      std::printf("\n");
    } else if (cmd == "kids") {
      size_t i;
      std::cin >> i >> num;
      const double v = std::strtod(num.c_str(), nullptr);
      const int a = h.take_slot(), b = h.take_slot();
      h.push(v, r.nodes.at(i).depth + 1, a);
      h.push(v, r.nodes.at(i).depth + 1, b);
      std::printf("slots %d %d\n", a, b);
    } else if (cmd == "requeue") {
      size_t i;
      std::cin >> i;
      NodeHeap::Node n = r.nodes.at(i);
      n.slot = h.take_slot();
      h.requeue(n);
      std::printf("slots %d\n", n.slot);
    } else if (cmd == "end") {
      std::printf("state %d %d\n", h.open(), h.hw());
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
