// Invariants of the lane-group list scheduler (csrc/rtg_group_sched.h), stand-alone and without a device:
//   group_sched_check [expected_steps p0 p1 ...]
// checks the built-in chains, stars and random trees and, when given, the tree p0 p1 ... (parents, root -1), whose
// schedule with a root entry on 4 lanes must take expected_steps.  For L = 4 and 8, with and without a root entry,
// over the whole tree and over ancestor-closed masks: every included joint appears exactly once and no other does; a
// parent sits at a strictly earlier step; no step is empty; the child links enumerate each joint's children
// ascending and completely.  Built and run by tests/test_host_logic.py.
#include "rtg_group_sched.h"

#include <cstdio>
#include <cstdlib>

static int failures = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            ++failures;                  \
            std::printf("FAIL " __VA_ARGS__); \
            std::printf("\n");           \
        }                                \
    } while (0)

static void check_schedule(const std::vector<int32_t> &par, const std::vector<char> *inc, bool root_entry, int L,
                           int expected_steps)
{
    const int J = (int)par.size();
    std::vector<int> order;
    const int steps = rtg::group_list_schedule(par.data(), J, inc ? inc->data() : nullptr, root_entry, L, J, order);
    CHECK(steps >= 0 && (int)order.size() == steps * L, "J=%d L=%d: %d steps, %zu entries", J, L, steps, order.size());
    if (expected_steps >= 0) CHECK(steps == expected_steps, "J=%d L=%d: %d steps, expected %d", J, L, steps, expected_steps);
    std::vector<int> step_of(J, -1);
    for (int s = 0; s < steps; ++s) {
        int busy = 0;
        for (int u = 0; u < L; ++u) {
            const int j = order[s * L + u];
            if (j < 0) continue;
            ++busy;
            CHECK(j < J && step_of[j] == -1, "J=%d L=%d: joint %d appears twice or is out of range", J, L, j);
            if (j < J) step_of[j] = s;
        }
        CHECK(busy > 0, "J=%d L=%d: step %d is empty", J, L, s);
    }
    for (int j = 0; j < J; ++j) {
        const bool want = (j == 0 ? root_entry : true) && (!inc || (*inc)[j]);
        CHECK((step_of[j] >= 0) == want, "J=%d L=%d: joint %d %s", J, L, j, want ? "is missing" : "should have no entry");
        if (j > 0 && step_of[j] >= 0 && (par[j] != 0 || root_entry))   // without an entry the root counts as done
            CHECK(step_of[par[j]] >= 0 && step_of[par[j]] < step_of[j],
                  "J=%d L=%d: joint %d at step %d, its parent %d at %d", J, L, j, step_of[j], par[j], step_of[par[j]]);
    }
}

static void check_tree(const std::vector<int32_t> &par, int expected_steps_l4)
{
    const int J = (int)par.size();
    std::vector<uint32_t> fc, ns;
    rtg::group_child_links(par.data(), J, fc, ns);
    for (int j = 0; j < J; ++j) {
        uint32_t c = fc[j];
        for (int k = j + 1; k < J; ++k)
            if (par[k] == j) {
                CHECK(c == (uint32_t)k, "J=%d: child links of %d give %u where child %d is next", J, j, c, k);
                c = c < (uint32_t)J ? ns[c] : 0xFF;
            }
        CHECK(c == 0xFF, "J=%d: child links of %d go on to %u past its last child", J, j, c);
    }
    for (int L : {4, 8})
        for (int root_entry = 0; root_entry < 2; ++root_entry) {
            check_schedule(par, nullptr, root_entry, L, root_entry && L == 4 ? expected_steps_l4 : -1);
            for (int k = 0; k < J; k += 1 + J / 5) {   // the ancestors of joints k, k + 7 and J - 1
                std::vector<char> inc(J, 0);
                for (int t : {k, (k + 7) % J, J - 1})
                    for (int a = t; a != -1 && !inc[a]; a = par[a]) inc[a] = 1;
                check_schedule(par, &inc, root_entry, L, -1);
            }
        }
}

int main(int argc, char **argv)
{
    int trees = 0;
    if (argc > 2) {
        std::vector<int32_t> par;
        for (int i = 2; i < argc; ++i) par.push_back(std::atoi(argv[i]));
        check_tree(par, std::atoi(argv[1]));
        ++trees;
    }
    for (int J : {1, 2, 36, 37, 64}) {
        std::vector<int32_t> chain(J), star(J);
        for (int j = 0; j < J; ++j) chain[j] = j - 1, star[j] = j ? 0 : -1;
        check_tree(chain, J);                  // a chain takes one step per joint
        check_tree(star, 1 + (J - 1 + 3) / 4); // a star: the root, then its J - 1 children four at a time
        trees += 2;
    }
    uint32_t seed = 12345;
    const auto rnd = [&]() { return (seed = seed * 1664525u + 1013904223u) >> 8; };
    for (int it = 0; it < 200; ++it, ++trees) {
        const int J = 1 + (int)(rnd() % 64);
        std::vector<int32_t> par(J, -1);
        for (int j = 1; j < J; ++j) par[j] = (int32_t)(rnd() % (uint32_t)j);
        check_tree(par, -1);
    }
    std::printf("group_sched_check: %d trees, %d failures\n", trees, failures);
    return failures != 0;
}
