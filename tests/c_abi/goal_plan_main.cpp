// The plan of a goal field launch (csrc/bcp_goal_plan.h: the route, the threads, the grid, the dynamic LDS and the scratch
// of every goal_field_kernel launch) on the host alone.  The header has no HIP in it; this program includes nothing else of
// the library and is built with -fsanitize=address,undefined by tests/test_goal_plan_host.py, which works the expected
// numbers out itself.
//   goal_plan_main ROWS,COLS,TRIPS,BOUND,COST,FORCED ...    prints per argument
//       "in_lds threads grid lds_bytes scratch_words", then "limits" and the header's constants, then "goal plan ok"
#include <cstdio>

#include "bcp_goal_plan.h"

using namespace bcp;

int main(int argc, char** argv)
{
    for (int i = 1; i < argc; ++i) {
        int rows, cols, bound, cost, forced;
        long long trips;
        if (sscanf(argv[i], "%d,%d,%lld,%d,%d,%d", &rows, &cols, &trips, &bound, &cost, &forced) != 6) return 2;
        const GoalPlan p = plan_goal(rows, cols, trips, bound != 0, cost != 0, forced != 0);
        printf("%d %u %lld %zu %lld\n", p.in_lds ? 1 : 0, p.threads, (long long)p.grid, p.lds_bytes, (long long)p.scratch_words);
    }
    printf("limits %zu %lld %lld %lld %lld %d\n", kGoalMaxLds, (long long)kGoalLdsGrid, (long long)kGoalBoundGrid,
           (long long)kGoalGlobalGrid, (long long)kGoalScratchBytes, kGoalFixedWords);
    printf("goal plan ok\n");
    return 0;
}
