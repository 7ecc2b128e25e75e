// work_layout.h — how every workspace is laid out: a layout function takes its fields from one WorkCarve in the order they lie,
// each with its OWN size beside it, and reads the total off the carver, so a field inserted or moved cannot overlap its neighbour.
#pragma once
#include <stddef.h>

namespace dcx {
struct WorkCarve {   // offsets of a workspace, each field 256-byte aligned; `at` is the total so far
    size_t at = 0;
    size_t take(size_t bytes) { const size_t off = at; at += (bytes + 255) / 256 * 256; return off; }   // the field's offset
    template <class T> size_t take_n(size_t n) { return take(n * sizeof(T)); }
};
}  // namespace dcx
