// The entry of a row map or position table that means "no row": a padding row of a panel, a tile outside a reach.
#pragma once
#include <stdint.h>

namespace bae {
static const uint32_t kNoneRow = 0xffffffffu;
}  // namespace bae
