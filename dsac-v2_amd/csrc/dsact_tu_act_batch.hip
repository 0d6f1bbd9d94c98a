// dsact_tu_act_batch.hip -- the batched acting forward of libdsact.so (dsact_act_batch.h); dsact_api.hip launches it through
// the declarations that header gives every other unit
#include <hip/hip_runtime.h>
#define DSACT_FAMILY_UNIT 1        // the non-template kernels of dsact_kernels.h are compiled in dsact_api.hip only
#define DSACT_ACT_BATCH_DEFINE 1
#include "dsact_act_batch.h"
