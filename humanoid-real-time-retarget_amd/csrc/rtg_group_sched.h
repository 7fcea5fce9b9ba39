// rtg_group_sched.h -- the host list scheduler of the lane-group tiles (rtg_fk_group.cuh).  Plain C++, no device: the
// topologies (rtg_fk.hip) and the retarget_to plans (rtg_retarget_to.hip) build their GEnt entries from its order, and
// tests/group_sched_check.cpp checks its invariants.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace rtg {

// List schedule of a parent-indexed tree (par[j] < j) on L lanes.  The joints scheduled are those with inc[j] (an
// ancestor-closed set; nullptr: all), the root only with root_entry (without, it counts as done before step 0).  A
// joint is ready once its parent's step is past; each step takes up to L ready joints, longest remaining chain
// (height) first, ties by index -- for a tree that is the critical-path bound (depth + 1 steps) whenever L covers the
// widest level the chains keep busy (Hu on 4 lanes: 10 steps for 31 joints).  The kernels' bits do not depend on it.
// Fills order with steps x L joints (-1: idle lane) and returns the step count, or -1 if it would exceed max_steps.
inline int group_list_schedule(const int32_t *par, int J, const char *inc, bool root_entry, int L, int max_steps,
                               std::vector<int> &order)
{
    const auto in = [&](int j) { return !inc || inc[j]; };
    std::vector<int> h(J, 1), done(J, -2);   // done: the joint's step; -2: not yet; -1: the root without an entry
    int todo = root_entry ? 1 : 0;
    if (!root_entry) done[0] = -1;
    for (int j = J - 1; j > 0; --j)
        if (in(j)) {
            h[par[j]] = std::max(h[par[j]], h[j] + 1);
            ++todo;
        }
    order.clear();
    int steps = 0, placed = 0;
    std::vector<int> ready;
    while (placed < todo) {
        if (steps >= max_steps) return -1;
        ready.clear();
        for (int j = 0; j < J; ++j)
            if (in(j) && done[j] == -2 && (j == 0 || (done[par[j]] != -2 && done[par[j]] < steps))) ready.push_back(j);
        std::stable_sort(ready.begin(), ready.end(), [&](int a, int b) { return h[a] > h[b]; });
        for (int u = 0; u < L; ++u) {
            const int j = u < (int)ready.size() ? ready[u] : -1;
            if (j >= 0) {
                done[j] = steps;
                ++placed;
            }
            order.push_back(j);
        }
        ++steps;
    }
    return steps;
}

// child links for the reverse sweep: each joint's first child and next sibling, by ascending index; 0xFF: none
inline void group_child_links(const int32_t *par, int J, std::vector<uint32_t> &first_child,
                              std::vector<uint32_t> &next_sibling)
{
    first_child.assign(J, 0xFF);
    next_sibling.assign(J, 0xFF);
    for (int j = J - 1; j > 0; --j) {
        next_sibling[j] = first_child[par[j]];
        first_child[par[j]] = (uint32_t)j;
    }
}

}  // namespace rtg
