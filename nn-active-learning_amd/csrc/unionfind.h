// The atomic-min union-find shared by the component kernels (ccl.hip, slic.hip): a forest in an int array with parent[x] <= x,
// so the root of a finished tree is the minimum of its set whatever order the workgroups ran in.  Visibility while a launch
// hooks trees: a word another workgroup may write is read only through the return value of an atomic or through a relaxed
// agent-scope atomic load (never a plain load, which another XCD's L2 or this CU's L1 may serve from a stale line).
#pragma once
#include <hip/hip_runtime.h>

namespace alq {

__device__ inline int cc_load(int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x while other workgroups hook trees (merge launch): every word through an agent-scope atomic load
__device__ inline int cc_find_live(int *parent, int x) {
    int p = cc_load(parent + x);
    while (p != x) {
        x = p;
        p = cc_load(parent + x);
    }
    return x;
}

// the root of x in a forest nobody hooks any more (after the merge launch)
__device__ inline int cc_find(const int *parent, int x) {
    int p = parent[x];
    while (p != x) {
        x = p;
        p = parent[x];
    }
    return x;
}

// -> a root-ward member of the united set (the next union of the same voxel starts there)
__device__ inline int cc_unite(int *parent, int a, int b) {
    for (;;) {
        a = cc_find_live(parent, a);
        b = cc_find_live(parent, b);
        if (a == b) return a;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        // b is (was) a root above a: hook it.  old != b: someone hooked b under `old` first - the minimum now stands in
        // parent[b], and the set of the other value still has to meet it: carry on with (a, old)
        const int old = atomicMin(parent + b, a);
        if (old == b) return a;
        b = old;
    }
}

}  // namespace alq
