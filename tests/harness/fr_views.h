// Views of plain fr arrays with the accessors the lb_fr.h / lb_fk20.h lane functions take (ld / st
// like the kernels' LDS and global views, operator() like their table readers), shared by the
// kzg_*_lanes.h headers.
#pragma once
#include "lb_fr.h"

struct fr_cview {  // read-only
  const fr* p;
  fr ld(uint32_t i) const { return p[i]; }
};
struct fr_view {  // read-write
  fr* p;
  fr ld(uint32_t i) const { return p[i]; }
  void st(uint32_t i, const fr& v) { p[i] = v; }
};
struct fr_table {
  const fr* p;
  fr operator()(uint32_t k) const { return p[k]; }
};
