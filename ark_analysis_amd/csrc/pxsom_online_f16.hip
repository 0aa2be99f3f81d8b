// pxsom_online_f16.hip -- the exact online SOM's kernels for binary16 rows (pxsom_online.h)
#include "pxsom_online.h"

template int pxsom::train_online<_Float16>(PXSOM_ONLINE_ARGS(_Float16));
