// unionfind.hpp -- the lock-free min-root union-find over 32-bit indices that points.hip (DBSCAN: the components of the core points) and
// mesh.hip (the components of a triangle mesh) share.  parent[x] <= x at all times (parent[x] == x: a root); a union hooks the LARGER root
// under the smaller with atomicCAS(parent + hi, hi, lo), so a root is hooked once and the root of a finished component is its smallest
// member.  Every access to parent[] while unions run is an agent-scope atomic -- a plain load may be served from a line another XCD's L2
// has since changed; kernels after them read it with plain loads behind the kernel boundary.
//
// Termination, independent of any other workgroup's progress:
//   cluster_find: the loop runs while parent[x] < x and moves x to that parent: x strictly decreases, at most n trips, and a value that
//     breaks parent[x] <= x ends the loop instead of extending it.  The atomicMin on the way (path halving: a node is pointed at its
//     grandparent) only lowers a parent to one of the node's ancestors: a root is never changed, nobody leaves its tree, and
//     parent[x] <= x stays.  Without it the trees of a chain-shaped cloud visited in chain order reach a depth of n.
//   cluster_unite: a trip ends the loop (same root, or the CAS hooked hi) or has OBSERVED parent[hi] < hi in the value the CAS returned
//     and goes on from the root found below that value, so max(a, b) strictly decreases from trip to trip: at most n trips, in fact
//     one per root that another thread hooked between this thread's find and its CAS.  Hooking under a lo that has meanwhile stopped
//     being a root is still a correct link (lo < hi, same component).  The loop is capped at CLUSTER_RETRY_CAP all the same; a thread
//     that hits the cap raises *err, the call then reports n_clusters = -1 and the host forms return SFMHIP_E_NUMERIC.  Nothing waits:
//     no thread reads a word in order to see another thread's write arrive.
#pragma once
#include <hip/hip_runtime.h>

typedef unsigned long long pu64;
typedef unsigned int pu32;

#define CLUSTER_RETRY_CAP (1 << 16)

__device__ __forceinline__ pu32 cluster_parent(pu32* parent, pu32 x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ pu32 cluster_find(pu32* parent, pu32 x)
{
    pu32 p = cluster_parent(parent, x);
    while (p < x) {
        const pu32 gp = cluster_parent(parent, p);
        if (gp < p) atomicMin(parent + x, gp);
        x = p; p = gp;
    }
    return x;
}

// unites the components of a and b; returns a member of that component no larger than the root found for a (the caller's next start)
__device__ __forceinline__ pu32 cluster_unite(pu32* parent, pu32 a, pu32 b, pu32* err)
{
    a = cluster_find(parent, a); b = cluster_find(parent, b);
    for (int trip = 0; trip < CLUSTER_RETRY_CAP; ++trip) {
        if (a == b) return a;
        const pu32 hi = a > b ? a : b, lo = a > b ? b : a;
        const pu32 old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return lo;
        a = cluster_find(parent, old); b = lo;             // old < hi: somebody else hooked hi first
    }
    __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return a;
}
