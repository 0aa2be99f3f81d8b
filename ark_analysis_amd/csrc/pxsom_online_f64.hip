// pxsom_online_f64.hip -- the exact online SOM's kernels for binary64 rows (pxsom_online.h)
#include "pxsom_online.h"

template int pxsom::train_online<double>(PXSOM_ONLINE_ARGS(double));
