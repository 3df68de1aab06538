// The size limit of the one-workgroup solves, shared by the kernels (tiny.hpp) and the host-only rules (sweep_rules.hpp).
#pragma once

namespace cfmm {

constexpr int TINY_N = 64;                 // tokens (and price groups): one per lane of wave 0

}  // namespace cfmm
