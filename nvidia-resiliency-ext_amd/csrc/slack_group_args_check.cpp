// slack_group_args_check.cpp -- a stand-alone host program for `make slack-group-args-check`: it drives the argument checks
// of nvrx_slack_group_score with INVALID arguments only, so no call reaches a device, and is meant to be built together with
// nvrx_straggler.hip with AddressSanitizer and UndefinedBehaviorSanitizer on the host code.  Exit status 0 when every call
// returned the error the header promises.
#include "args_check.h"

int main() {
    float *slack = reinterpret_cast<float *>(uintptr_t{4096});  // never dereferenced: every call below fails its checks
    float *table = reinterpret_cast<float *>(uintptr_t{8192});
    int32_t *groups = reinterpret_cast<int32_t *>(uintptr_t{12288});
    void *out = reinterpret_cast<void *>(uintptr_t{16384});
    void *odd = reinterpret_cast<void *>(uintptr_t{16392});
    // (slack, table, R, K, S, groups, G, max_group, min_ranks, min_peers, out, stream)
    expect("R 0", nvrx_slack_group_score(slack, table, 0, 5, 2, groups, 1, 1, 4, 2, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("R < 0", nvrx_slack_group_score(slack, table, -3, 5, 2, groups, 1, 1, 4, 2, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("K < 0", nvrx_slack_group_score(slack, table, 8, -1, 2, groups, 2, 4, 4, 2, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("S < 0", nvrx_slack_group_score(slack, table, 8, 5, -1, groups, 2, 4, 4, 2, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("R too large", nvrx_slack_group_score(slack, table, NVRX_ROBUST_MAX_RANKS + 1, 5, 2, groups, 2, 4, 4, 2, out, nullptr),
           NVRX_ERR_RANGE, "ranks");
    expect("K too large", nvrx_slack_group_score(slack, table, 8, NVRX_MAX_ROWS + 1, 2, groups, 2, 4, 4, 2, out, nullptr), NVRX_ERR_RANGE, "ids");
    expect("S too large", nvrx_slack_group_score(slack, table, 8, 5, NVRX_MAX_ROWS + 1, groups, 2, 4, 4, 2, out, nullptr), NVRX_ERR_RANGE, "ids");
    expect("min_ranks 0", nvrx_slack_group_score(slack, table, 8, 5, 2, groups, 2, 4, 0, 2, out, nullptr), NVRX_ERR_RANGE, "min_ranks");
    expect("min_ranks < 0", nvrx_slack_group_score(slack, table, 8, 5, 2, groups, 2, 4, -4, 2, out, nullptr), NVRX_ERR_RANGE, "min_ranks");
    expect("null rows", nvrx_slack_group_score(nullptr, table, 8, 5, 2, groups, 2, 4, 4, 2, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null table", nvrx_slack_group_score(slack, nullptr, 8, 5, 2, groups, 2, 4, 4, 2, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null records", nvrx_slack_group_score(slack, table, 8, 5, 2, groups, 2, 4, 4, 2, nullptr, nullptr), NVRX_ERR_INVALID, "null");
    expect("null records, K 0", nvrx_slack_group_score(slack, nullptr, 8, 0, 2, groups, 2, 4, 4, 2, nullptr, nullptr), NVRX_ERR_INVALID, "null");
    expect("misaligned rows", nvrx_slack_group_score(reinterpret_cast<float *>(uintptr_t{4100}), table, 8, 5, 2, groups, 2, 4, 4, 2, out, nullptr),
           NVRX_ERR_INVALID, "aligned");
    expect("misaligned records", nvrx_slack_group_score(slack, table, 8, 5, 2, groups, 2, 4, 4, 2, odd, nullptr), NVRX_ERR_INVALID, "aligned");
    // the slack checks come first: a bad shape is reported even where the groups are wrong too
    expect("R 0 before G 0", nvrx_slack_group_score(slack, table, 0, 5, 2, groups, 0, 0, 4, 0, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("G 0", nvrx_slack_group_score(slack, table, 8, 5, 2, groups, 0, 4, 4, 2, out, nullptr), NVRX_ERR_INVALID, "groups");
    expect("G < 0", nvrx_slack_group_score(slack, table, 8, 5, 2, groups, -1, 4, 4, 2, out, nullptr), NVRX_ERR_INVALID, "groups");
    expect("G > R", nvrx_slack_group_score(slack, table, 8, 5, 2, groups, 9, 4, 4, 2, out, nullptr), NVRX_ERR_RANGE, "groups");
    expect("G too large", nvrx_slack_group_score(slack, table, NVRX_PEER_MAX_GROUPS + 2, 5, 2, groups, NVRX_PEER_MAX_GROUPS + 1, 4, 4, 2, out,
                                                 nullptr), NVRX_ERR_RANGE, "at most");
    expect("G before max_group", nvrx_slack_group_score(slack, table, 8, 5, 2, groups, 0, 0, 4, 0, out, nullptr), NVRX_ERR_INVALID, "groups");
    expect("max_group 0", nvrx_slack_group_score(slack, table, 8, 5, 2, groups, 2, 0, 4, 2, out, nullptr), NVRX_ERR_RANGE, "max_group");
    expect("max_group < 0", nvrx_slack_group_score(slack, table, 8, 5, 2, groups, 2, -4, 4, 2, out, nullptr), NVRX_ERR_RANGE, "max_group");
    expect("max_group > R", nvrx_slack_group_score(slack, table, 8, 5, 2, groups, 2, 9, 4, 2, out, nullptr), NVRX_ERR_RANGE, "max_group");
    expect("max_group before min_peers", nvrx_slack_group_score(slack, table, 8, 5, 2, groups, 2, 9, 4, 0, out, nullptr), NVRX_ERR_RANGE,
           "max_group");
    expect("min_peers 0", nvrx_slack_group_score(slack, table, 8, 5, 2, groups, 2, 4, 4, 0, out, nullptr), NVRX_ERR_RANGE, "min_peers");
    expect("min_peers < 0", nvrx_slack_group_score(slack, table, 8, 5, 2, groups, 2, 4, 4, -1, out, nullptr), NVRX_ERR_RANGE, "min_peers");
    expect("null groups", nvrx_slack_group_score(slack, table, 8, 5, 2, nullptr, 2, 4, 4, 2, out, nullptr), NVRX_ERR_INVALID, "null");
    printf("slack_group_args_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
