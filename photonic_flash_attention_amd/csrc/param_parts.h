// param_parts.h -- how the kernels over a KV cache compose their one argument block: a base struct every instantiation takes and one
// small part struct per mode flag, derived from in the flags' order.  A flag that is off contributes an empty base, so an instantiation
// without the mode keeps the block -- and the kernel arguments -- it had.
#pragma once
#include <type_traits>

namespace pfa {

// the place of a part that is switched off: empty, and a type of its own per part so that no two empty bases meet at one address
template <typename Part>
struct NoPart {};
template <bool ON, typename Part>
using PartIf = std::conditional_t<ON, Part, NoPart<Part>>;

// A part that ends in padding derives from this: a struct with a base is not a plain aggregate to the ABI, which then lets the next part
// start inside that padding -- where the member stood when the blocks were a chain of derived structs.  The offsets are in the kernels'
// code (tools/isa_same.py compares them).
struct TailPaddingReused {};

}  // namespace pfa
