// the hier_linear_regression device model (models/hier_glm.h): kernels for the one-wavefront geometries + registry entry
#include "models/hier_glm.h"
#define WN_MODEL_ID 15
#define WN_MODEL_TAG hier_linear_regression
#define WN_MODEL_TYPE wn::HierLinearRegressionModel
#include "wn_kernels.inc"
