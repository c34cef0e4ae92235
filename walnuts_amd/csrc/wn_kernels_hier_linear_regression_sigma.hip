// the hier_linear_regression_sigma device model (models/hier_scale_glm.h): kernels for the one-wavefront geometries + registry entry
#include "models/hier_scale_glm.h"
#define WN_MODEL_ID 35
#define WN_MODEL_TAG hier_linear_regression_sigma
#define WN_MODEL_TYPE wn::HierLinearRegressionSigmaModel
#include "wn_kernels.inc"
