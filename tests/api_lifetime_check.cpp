// The handle constructors of the C ABI on a machine without a device, for a run under ASan / UBSan
// (tests/test_api_lifetime_host.py): each constructor that can be given valid arguments there is called twice and must
// fail at its first device call with nothing leaked and *out left NULL; the two that need a live topology are called
// with NULL ones; every destructor takes NULL.  Prints one line per call: "<name> <status> <message>".
#include <cstdint>
#include <cstdio>

#include "rtg.h"

static int bad = 0;

static void report(const char *name, int rc, const void *out)
{
    std::printf("%s %d %s\n", name, rc, rc == RTG_OK ? "" : rtg_last_error());
    if (rc != RTG_OK && out) {
        std::printf("%s left *out set after a failure\n", name);
        bad = 1;
    }
}

int main()
{
    if (rtg_device_count() != 0) {
        std::printf("a device is visible: this program checks the no-device failure path\n");
        return 2;
    }
    const int32_t parents[3] = {-1, 0, 1};
    const float local_t[9] = {0.f, 0.f, 0.f, 0.1f, 0.f, 0.f, 0.f, 0.2f, 0.f};
    const float quat[12] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    const int32_t src[3] = {2, 1, 0};
    const int64_t start[2] = {0, 4};
    const int32_t len[2] = {4, 3};
    const float fps[2] = {30.f, 60.f};
    static float zero_pose[59 * 3];
    for (int i = 0; i < 59 * 3; ++i) zero_pose[i] = 0.01f * (float)i;
    int32_t parents21[21];
    for (int j = 0; j < 21; ++j) parents21[j] = j - 1;
    const int32_t axis[2] = {0, 1};

    for (int rep = 0; rep < 2; ++rep) {
        rtg_topology_t t = nullptr;
        report("rtg_topology_create", rtg_topology_create(parents, local_t, quat, 3, &t), t);
        rtg_motion_lib_t ml = nullptr;
        report("rtg_motion_lib_create", rtg_motion_lib_create(start, len, fps, 2, 8, &ml), ml);
        rtg_rot_ingest_t ri = nullptr;
        report("rtg_rot_ingest_create", rtg_rot_ingest_create(3, 3, src, quat, quat, &ri), ri);
        const struct { int kind, Js; } solvers[4] = {{RTG_SOLVER_FULL_BODY_POS, 59}, {RTG_SOLVER_UPPER_BODY, 21},
                                                     {RTG_SOLVER_FULL_BODY_ROT, 59}, {RTG_SOLVER_BODY_ROT, 21}};
        for (const auto &k : solvers) {
            rtg_solver_t s = nullptr;
            report("rtg_solver_create", rtg_solver_create(k.kind, zero_pose, zero_pose, parents21, k.Js, rep, &s), s);
        }
        // these two need a live topology, which needs a device: their checks, then out
        rtg_dof_model_t m = nullptr;
        report("rtg_dof_model_create(NULL)", rtg_dof_model_create(nullptr, axis, nullptr, nullptr, &m), m);
        rtg_retarget_plan_t p = nullptr;
        report("rtg_retarget_plan_create(NULL)",
               rtg_retarget_plan_create(nullptr, nullptr, src, src, 3, quat, local_t, quat, local_t, quat, 1.0f, &p), p);
        float *inbox = nullptr;
        report("rtg_server_inbox_alloc", rtg_server_inbox_alloc(&inbox), inbox);
    }
    report("rtg_topology_destroy(NULL)", rtg_topology_destroy(nullptr), nullptr);
    report("rtg_dof_model_destroy(NULL)", rtg_dof_model_destroy(nullptr), nullptr);
    report("rtg_retarget_plan_destroy(NULL)", rtg_retarget_plan_destroy(nullptr), nullptr);
    report("rtg_solver_destroy(NULL)", rtg_solver_destroy(nullptr), nullptr);
    report("rtg_server_inbox_free(NULL)", rtg_server_inbox_free(nullptr), nullptr);
    rtg_rot_ingest_destroy(nullptr);
    rtg_motion_lib_destroy(nullptr);
    std::printf("void destructors took NULL\n");
    return bad;
}
