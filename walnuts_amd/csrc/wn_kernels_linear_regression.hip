// the linear_regression device model (models/glm.h): kernels for the one-wavefront geometries + registry entry
#include "models/glm.h"
#define WN_MODEL_ID 4
#define WN_MODEL_TAG linear_regression
#define WN_MODEL_TYPE wn::LinearRegressionModel
#include "wn_kernels.inc"
