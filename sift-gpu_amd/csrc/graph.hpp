// graph.hpp -- the context's hipGraph cache: up to four captured compute
// sequences, evicted first in first out (a hit does not refresh an entry).
#pragma once

#include "ctx.hpp"

namespace sift {

// Appends the bytes of each value to a cache key.
template <typename... T>
void key_put(std::vector<char>& k, const T&... v) {
  (k.insert(k.end(), reinterpret_cast<const char*>(&v), reinterpret_cast<const char*>(&v) + sizeof(T)), ...);
}

inline void drop_graphs(sift_ctx* c) {
  for (auto& g : c->graphs) {
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (g.graph) (void)hipGraphDestroy(g.graph);
  }
  c->graphs.clear();
}

inline bool graphs_enabled(const sift_ctx* c) {
  return !(c->flags & (SIFT_FLAG_PROFILE | SIFT_FLAG_VERBOSE | SIFT_FLAG_NO_GRAPH));
}

// Runs body() on the context stream: replayed from a cached hipGraph when one
// was captured for the same key and buffers; captured now otherwise (direct
// launches if graphs are off or capture fails).  A caller whose buffers move
// between calls (a caching allocator, a ring of output slots) with the same
// shape gets the new capture patched into the cached executable with
// hipGraphExecUpdate -- no re-instantiation -- so a rotating set of buffers
// does not thrash the 4-entry cache.
template <typename F>
int run_graphed(sift_ctx* c, const std::vector<char>& key, const std::vector<char>& ptrs, F&& body) {
  auto direct = [&]() -> int {
    body();
    HIP_TRY(c, hipGetLastError());
    return SIFT_OK;
  };
  if (!graphs_enabled(c)) return direct();
  for (size_t i = 0; i < c->graphs.size(); ++i)
    if (c->graphs[i].key == key && c->graphs[i].ptrs == ptrs) {
      HIP_TRY(c, hipGraphLaunch(c->graphs[i].exec, c->stream));
      return SIFT_OK;
    }
  hipGraph_t g = nullptr;
  if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    return direct();
  }
  body();
  const hipError_t le = hipGetLastError();
  const hipError_t ce = hipStreamEndCapture(c->stream, &g);
  if (le != hipSuccess || ce != hipSuccess || !g) {
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    return direct();  // capture failed: nothing ran, launch directly
  }
  c->graph_captures++;
  // same shape, other buffers: update the cached executable in place
  for (size_t i = 0; i < c->graphs.size(); ++i) {
    sift_ctx::GraphEntry& e = c->graphs[i];
    if (e.key != key) continue;
    hipGraphNode_t err_node = nullptr;
    hipGraphExecUpdateResult res;
    if (hipGraphExecUpdate(e.exec, g, &err_node, &res) == hipSuccess && res == hipGraphExecUpdateSuccess) {
      (void)hipGraphDestroy(e.graph);
      e.graph = g;
      e.ptrs = ptrs;
      c->graph_updates++;
      HIP_TRY(c, hipGraphLaunch(e.exec, c->stream));
      return SIFT_OK;
    }
    // not updatable: the update may have patched some nodes before it
    // failed, so this executable no longer matches its recorded buffers --
    // drop the entry and instantiate a new executable below
    (void)hipGetLastError();
    (void)hipGraphExecDestroy(e.exec);
    (void)hipGraphDestroy(e.graph);
    c->graphs.erase(c->graphs.begin() + (long)i);
    break;
  }
  sift_ctx::GraphEntry e;
  e.key = key;
  e.ptrs = ptrs;
  e.graph = g;
  if (hipGraphInstantiate(&e.exec, e.graph, nullptr, nullptr, 0) != hipSuccess) {
    (void)hipGraphDestroy(e.graph);
    (void)hipGetLastError();
    return direct();
  }
  c->graph_instantiations++;
  if (c->graphs.size() >= 4) {
    (void)hipGraphExecDestroy(c->graphs.front().exec);
    (void)hipGraphDestroy(c->graphs.front().graph);
    c->graphs.erase(c->graphs.begin());
  }
  c->graphs.push_back(e);
  HIP_TRY(c, hipGraphLaunch(e.exec, c->stream));
  return SIFT_OK;
}

}  // namespace sift
