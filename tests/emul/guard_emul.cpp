// guard_emul.cpp -- the exception guard of the C entry points (mhx::guarded, mhx_internal.h) on its own, as a host program
// built with AddressSanitizer and UBSan: what a throwing body turns into, code and message byte for byte, and that a
// body's own result passes through.  Linked with mhx_text.cpp, the home of fail() and of the message it leaves.
#include <stdio.h>
#include <string.h>

#include <new>
#include <stdexcept>

#include "../../auriclass_amd/csrc/mhx_internal.h"

static int check(const char *what, int got, int want_code, const char *want_text)
{
    const char *text = mhx_last_error();
    if (got == want_code && strcmp(text, want_text) == 0) return 0;
    printf("%s: code %d (want %d), message \"%s\" (want \"%s\")\n", what, got, want_code, text, want_text);
    return 1;
}

int main()
{
    int bad = 0;
    mhx::clear_error();
    bad += check("bad_alloc", mhx::guarded("NAME", []() -> int { throw std::bad_alloc(); }), MHX_E_INTERNAL, "NAME: out of host memory");
    mhx::clear_error();
    bad += check("runtime_error", mhx::guarded("NAME", []() -> int { throw std::runtime_error("x"); }), MHX_E_INTERNAL, "NAME: x");
    mhx::clear_error();
    bad += check("result", mhx::guarded("NAME", [] { return 7; }), 7, ""); // nothing thrown: the body's code, no message
    if (bad) return 1;
    printf("ok 3\n");
    return 0;
}
