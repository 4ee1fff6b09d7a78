// offpolicy_unit.hip -- one translation unit for the off-policy dense engine, replay sampling and the fused-step executor: its phase kernels (exec.hip) call
// the op bodies defined in dense.hip, sac.hip and per.hip (cql.hip, iq.hip, advil.hip, asaf.hip, gail_off.hip and nda_gail.hip use the dense engine's and sac.hip's helpers and share chain.h's host-side step and chain scaffolding), and device code is not linked across translation units in this build.
#include "dense.hip"
#include "sac.hip"
#include "chain.h"
#include "cql.hip"
#include "iq.hip"
#include "advil.hip"
#include "asaf.hip"
#include "gail_off.hip"
#include "nda_gail.hip"
#include "train_dense.hip"
#include "per.hip"
#include "exec.hip"
