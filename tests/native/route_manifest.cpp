// route_manifest.cpp -- a second main for launch_recorder.cpp (built with -DSQLLM_RECORDER_NO_MAIN): plans the cases it reads
// from stdin through the host layer and prints every launch with every field (rec_trace), so that a test can check which
// launcher, and which instantiation of it, a labelled route really reaches.  No GPU, nothing is launched; operand pointers are
// fake.  Built and fed by tests/test_precision_cpu.py::test_route_manifest with the route table of tests/test_gpu_precision.py.
//
// One case per line, fields separated by blanks:
//   <id> <ws|null> <bits> <K> <batch> <n_ops> <N,nnz,topX> x n_ops  [<option>=<value> ...]
// "ws": sqllm_launch_group_ws with an ample workspace (what the Python module and a pass with a workspace do), "null": the same
// entry point without one.  Options are set for the case and put back afterwards.  Output: "begin <id>", the launches,
// "end <id> rc=<code>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "sqllm_hip.h"

extern bool rec_trace;

int main() {
  rec_trace = true;
  if (sqllm_set_option("cu_count", 256) != SQLLM_OK) return 2;
  char buf[4096];
  while (fgets(buf, sizeof(buf), stdin)) {
    std::istringstream in(buf);
    std::string id, entry, tok;
    int bits = 0, K = 0, batch = 0, n_ops = 0;
    if (!(in >> id >> entry >> bits >> K >> batch >> n_ops)) continue;
    if (n_ops < 1 || n_ops > 4) return 3;
    sqllm_op ops[4];
    memset(ops, 0, sizeof(ops));
    for (int i = 0; i < n_ops; ++i) {
      int N = 0, nnz = 0, topX = 0;
      if (!(in >> tok) || sscanf(tok.c_str(), "%d,%d,%d", &N, &nnz, &topX) != 3) return 3;
      sqllm_op& op = ops[i];
      const uintptr_t base = 0x100000u * (uintptr_t)(i + 1);
      op.bits = bits;
      op.batch = batch;
      op.K = K;
      op.N = N;
      op.vec = reinterpret_cast<const float*>((uintptr_t)0x1000);  // (the ops of a group share vec)
      op.qweight = reinterpret_cast<const int32_t*>(base + 0x2000);
      op.mul = reinterpret_cast<float*>(base + 0x3000);
      op.lookup_table = reinterpret_cast<const float*>(base + 0x4000);
      if (nnz > 0) {
        op.rows = reinterpret_cast<const int32_t*>(base + 0x5000);
        op.cols = reinterpret_cast<const int32_t*>(base + 0x6000);
        op.vals = reinterpret_cast<const float*>(base + 0x7000);
        op.nnz = nnz;
      }
      if (topX > 0) {
        op.full_rows = reinterpret_cast<const float*>(base + 0x8000);
        op.full_row_indices = reinterpret_cast<const int32_t*>(base + 0x9000);
        op.topX = topX;
      }
    }
    std::vector<std::pair<std::string, int>> saved;
    while (in >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) return 3;
      const std::string name = tok.substr(0, eq);
      int old = 0;
      if (sqllm_get_option(name.c_str(), &old) != SQLLM_OK) return 4;
      saved.emplace_back(name, old);
      if (sqllm_set_option(name.c_str(), atoi(tok.c_str() + eq + 1)) != SQLLM_OK) return 4;
    }
    printf("begin %s\n", id.c_str());
    const bool ws = entry == "ws";
    const int rc = sqllm_launch_group_ws(ops, n_ops, ws ? reinterpret_cast<void*>((uintptr_t)0x40000000) : nullptr, ws ? (1ll << 40) : 0, nullptr);
    printf("end %s rc=%d\n", id.c_str(), rc);
    for (auto it = saved.rbegin(); it != saved.rend(); ++it) sqllm_set_option(it->first.c_str(), it->second);
  }
  return 0;
}
