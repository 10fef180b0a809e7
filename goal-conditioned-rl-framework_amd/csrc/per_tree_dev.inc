// per_tree_dev.inc — the device side of the priority tree that its units share: the view of a tree a kernel takes by value, the
// ONE fixed reduction order of a node (the whole contract of the tree: tests/per_tree_ref.py reduce64), the recomputation of a range
// of nodes, and the host's view_of.  Included INSIDE the including unit's anonymous namespace (per_tree.hip, her_td.hip), behind
// `using gcrl::kPerFan; using gcrl::kPerMaxLevels;`, so that each unit's kernels keep their internal names.

struct TreeView {
  float* tree;
  long long off[kPerMaxLevels];
  int levels;
};

__device__ inline float wave_sum64(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;   // the same bits in every lane (a + b == b + a)
}

// the entries [x0, x1) of level k - 1 changed: recompute their parents on level k; one wave per node
__device__ inline void reduce_range(const TreeView& t, int k, long long p0, long long p1, int wave, int nwaves, int lane) {
  const float* child = t.tree + t.off[k - 1];
  float* parent = t.tree + t.off[k];
  for (long long node = p0 + wave; node < p1; node += nwaves) {
    const float s = wave_sum64(child[node * kPerFan + lane]);
    if (lane == 0) parent[node] = s;
  }
}

inline TreeView view_of(const gcrl_per_tree* t) {
  TreeView v;
  v.tree = t->tree;
  for (int k = 0; k < kPerMaxLevels; ++k) v.off[k] = t->L.off[k];
  v.levels = t->L.levels;
  return v;
}
