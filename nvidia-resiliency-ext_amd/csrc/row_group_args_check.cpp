// row_group_args_check.cpp -- a stand-alone host program for `make row-group-args-check`: it drives the argument checks of
// nvrx_rowfam_group_score with INVALID arguments only, so no call reaches a device, and is meant to be built together with
// nvrx_straggler.hip with AddressSanitizer and UndefinedBehaviorSanitizer on the host code.  Exit status 0 when every call
// returned the error the header promises.
#include "args_check.h"

static void expect_words(const char *what, size_t got, size_t want) {
    if (got != want) {
        fprintf(stderr, "FAIL %s: %zu words (want %zu)\n", what, got, want);
        failures++;
    }
}

int main() {
    float *planes = reinterpret_cast<float *>(uintptr_t{4096});  // never dereferenced: every call below fails its checks
    float *table = reinterpret_cast<float *>(uintptr_t{8192});
    int32_t *groups = reinterpret_cast<int32_t *>(uintptr_t{12288});
    void *out = reinterpret_cast<void *>(uintptr_t{16384});
    void *odd = reinterpret_cast<void *>(uintptr_t{16392});
    // (planes, n_planes, table, R, K, S, groups, G, first_rank, n_ranks, min_ranks, out, stream)
    expect("R 0", nvrx_rowfam_group_score(planes, 1, table, 0, 5, 2, groups, 1, 0, 1, 2, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("R < 0", nvrx_rowfam_group_score(planes, 1, table, -3, 5, 2, groups, 1, 0, 1, 2, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("K < 0", nvrx_rowfam_group_score(planes, 1, table, 8, -1, 2, groups, 2, 0, 8, 2, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("S < 0", nvrx_rowfam_group_score(planes, 1, table, 8, 5, -1, groups, 2, 0, 8, 2, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("R too large", nvrx_rowfam_group_score(planes, 1, table, NVRX_ROBUST_MAX_RANKS + 1, 5, 2, groups, 2, 0, 8, 2, out, nullptr),
           NVRX_ERR_RANGE, "ranks");
    expect("K too large", nvrx_rowfam_group_score(planes, 1, table, 8, NVRX_MAX_ROWS + 1, 2, groups, 2, 0, 8, 2, out, nullptr), NVRX_ERR_RANGE, "ids");
    expect("S too large", nvrx_rowfam_group_score(planes, 1, table, 8, 5, NVRX_MAX_ROWS + 1, groups, 2, 0, 8, 2, out, nullptr), NVRX_ERR_RANGE, "ids");
    expect("first_rank < 0", nvrx_rowfam_group_score(planes, 1, table, 8, 5, 2, groups, 2, -1, 4, 2, out, nullptr), NVRX_ERR_RANGE, "outside");
    expect("n_ranks 0", nvrx_rowfam_group_score(planes, 1, table, 8, 5, 2, groups, 2, 0, 0, 2, out, nullptr), NVRX_ERR_RANGE, "outside");
    expect("ranks past R", nvrx_rowfam_group_score(planes, 1, table, 8, 5, 2, groups, 2, 5, 4, 2, out, nullptr), NVRX_ERR_RANGE, "outside");
    expect("planes 0", nvrx_rowfam_group_score(planes, 0, table, 8, 5, 2, groups, 2, 0, 8, 2, out, nullptr), NVRX_ERR_RANGE, "planes");
    expect("planes < 0", nvrx_rowfam_group_score(planes, -1, table, 8, 5, 2, groups, 2, 0, 8, 2, out, nullptr), NVRX_ERR_RANGE, "planes");
    expect("planes too large", nvrx_rowfam_group_score(planes, NVRX_EPISODE_PLANES + 1, table, 8, 5, 2, groups, 2, 0, 8, 2, out, nullptr),
           NVRX_ERR_RANGE, "planes");
    expect("min_ranks 0", nvrx_rowfam_group_score(planes, 1, table, 8, 5, 2, groups, 2, 0, 8, 0, out, nullptr), NVRX_ERR_RANGE, "min_ranks");
    expect("min_ranks < 0", nvrx_rowfam_group_score(planes, 1, table, 8, 5, 2, groups, 2, 0, 8, -2, out, nullptr), NVRX_ERR_RANGE, "min_ranks");
    expect("G 0", nvrx_rowfam_group_score(planes, 1, table, 8, 5, 2, groups, 0, 0, 8, 2, out, nullptr), NVRX_ERR_INVALID, "groups");
    expect("G < 0", nvrx_rowfam_group_score(planes, 1, table, 8, 5, 2, groups, -1, 0, 8, 2, out, nullptr), NVRX_ERR_INVALID, "groups");
    expect("G > R", nvrx_rowfam_group_score(planes, 1, table, 8, 5, 2, groups, 9, 0, 8, 2, out, nullptr), NVRX_ERR_RANGE, "groups");
    expect("G too large", nvrx_rowfam_group_score(planes, 1, table, NVRX_PEER_MAX_GROUPS + 2, 5, 2, groups, NVRX_PEER_MAX_GROUPS + 1, 0, 8, 2,
                                                  out, nullptr), NVRX_ERR_RANGE, "at most");
    expect("null planes", nvrx_rowfam_group_score(nullptr, 1, table, 8, 5, 2, groups, 2, 0, 8, 2, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null table at K > 0", nvrx_rowfam_group_score(planes, 1, nullptr, 8, 5, 2, groups, 2, 0, 8, 2, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null groups", nvrx_rowfam_group_score(planes, 1, table, 8, 5, 2, nullptr, 2, 0, 8, 2, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null groups at K 0", nvrx_rowfam_group_score(planes, 1, nullptr, 8, 0, 2, nullptr, 2, 0, 8, 2, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null records", nvrx_rowfam_group_score(planes, 1, table, 8, 5, 2, groups, 2, 0, 8, 2, nullptr, nullptr), NVRX_ERR_INVALID, "null");
    expect("misaligned records", nvrx_rowfam_group_score(planes, 1, table, 8, 5, 2, groups, 2, 0, 8, 2, odd, nullptr), NVRX_ERR_INVALID, "aligned");
    expect("misaligned records at K 0", nvrx_rowfam_group_score(planes, 7, nullptr, 8, 0, 2, groups, 2, 0, 8, 2, odd, nullptr), NVRX_ERR_INVALID, "aligned");
    // the order: a bad shape wins over a bad rank range, that over planes, that over min_ranks, that over G, that over the pointers
    expect("shape before ranks", nvrx_rowfam_group_score(nullptr, 0, nullptr, 0, 5, 2, nullptr, 0, 5, 4, 0, odd, nullptr), NVRX_ERR_INVALID, "shape");
    expect("ranks before planes", nvrx_rowfam_group_score(nullptr, 0, nullptr, 8, 5, 2, nullptr, 0, 5, 4, 0, odd, nullptr), NVRX_ERR_RANGE, "outside");
    expect("planes before min_ranks", nvrx_rowfam_group_score(nullptr, 0, nullptr, 8, 5, 2, nullptr, 0, 0, 8, 0, odd, nullptr), NVRX_ERR_RANGE, "planes");
    expect("min_ranks before G", nvrx_rowfam_group_score(nullptr, 1, nullptr, 8, 5, 2, nullptr, 0, 0, 8, 0, odd, nullptr), NVRX_ERR_RANGE, "min_ranks");
    expect("G before pointers", nvrx_rowfam_group_score(nullptr, 1, nullptr, 8, 5, 2, nullptr, 9, 0, 8, 2, odd, nullptr), NVRX_ERR_RANGE, "groups");
    expect("null before misaligned", nvrx_rowfam_group_score(nullptr, 1, table, 8, 5, 2, groups, 2, 0, 8, 2, odd, nullptr), NVRX_ERR_INVALID, "null");

    // the size: the function and the macro agree; a negative argument has no size
    expect_words("words 2x(3+4), 5 ranks", nvrx_rowfam_group_words(2, 3, 4, 5), NVRX_ROWFAM_GROUP_WORDS(2, 3, 4, 5));
    expect_words("words by hand", nvrx_rowfam_group_words(2, 3, 4, 5), 4 * 2 * 7 + 5 * 5);
    expect_words("words at K+S 0", nvrx_rowfam_group_words(3, 0, 0, 4), 4);
    expect_words("words at the limits", nvrx_rowfam_group_words(NVRX_PEER_MAX_GROUPS, NVRX_MAX_ROWS, NVRX_MAX_ROWS, NVRX_ROBUST_MAX_RANKS),
                 NVRX_ROWFAM_GROUP_WORDS(NVRX_PEER_MAX_GROUPS, NVRX_MAX_ROWS, NVRX_MAX_ROWS, NVRX_ROBUST_MAX_RANKS));
    expect_words("words G < 0", nvrx_rowfam_group_words(-1, 3, 4, 5), 0);
    expect_words("words K < 0", nvrx_rowfam_group_words(2, -3, 4, 5), 0);
    expect_words("words S < 0", nvrx_rowfam_group_words(2, 3, -4, 5), 0);
    expect_words("words n_ranks < 0", nvrx_rowfam_group_words(2, 3, 4, -5), 0);
    printf("row_group_args_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
