// args_check.h -- what the stand-alone *_args_check.cpp programs share (`make <name>-args-check`): each drives the argument
// checks of its entry points with INVALID arguments only, so no call reaches a device, and is built together with
// nvrx_straggler.hip with AddressSanitizer and UndefinedBehaviorSanitizer on the host code.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "nvrx_straggler.h"

static int failures = 0;

// the call returned `want` and left a message that holds `needle`
static void expect(const char *what, int got, int want, const char *needle) {
    const char *msg = nvrx_last_error();
    if (got != want || (needle && (!msg || !strstr(msg, needle)))) {
        fprintf(stderr, "FAIL %s: returned %d (want %d), message \"%s\" (want \"%s\")\n", what, got, want, msg ? msg : "", needle ? needle : "");
        failures++;
    }
}
