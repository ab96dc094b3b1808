// base_code_check.cpp -- kdf_base_code (csrc/kdf_text.h) as a host compiler sees it: prints the code of every byte value,
// one line of 256 numbers, for tests/test_base_code_host.py to hold against the Python key codec.  Host only.
#include <stdio.h>
#include "kdf_text.h"

int main() {
    for (uint32_t c = 0; c < 256; ++c) printf("%u%c", kdf_base_code(c), c == 255 ? '\n' : ' ');
    return 0;
}
