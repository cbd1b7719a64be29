// One group of kernels of liblodestar_bls.so, compiled once per group with -DLB_KGROUP=g
// (tools/gen_kdecls.py GROUPS); the host units (lb_engine.hip, lb_kzg_host.hip) launch
// them through lb_kdecl.h.
#define LB_KDECL_INSTANTIATE
#include "lb_kernels.h"
#include "lb_kzg.h"
#include "lb_kzg_field.h"
#include "lb_kzg_fk20.h"
#include "lb_kdecl.h"
