// pxsom_online_f32.hip -- the exact online SOM's kernels for binary32 rows (pxsom_online.h)
#include "pxsom_online.h"

template int pxsom::train_online<float>(PXSOM_ONLINE_ARGS(float));
