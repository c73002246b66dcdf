// oracle/ref_shim/SkyRegionDetect.h -- shadows the reference's header of the same name on the include path when its device code
// is compiled for the host (oracle/Makefile target `ref`).  Everything is in cuda_standin.h; see there.
#ifndef MPMVS_REF_SHIM_SKYREGIONDETECT_H_
#define MPMVS_REF_SHIM_SKYREGIONDETECT_H_
#include "cuda_standin.h"
#endif
