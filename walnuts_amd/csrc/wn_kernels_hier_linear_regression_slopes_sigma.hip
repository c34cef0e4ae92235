// the hier_linear_regression_slopes_sigma device model (models/hier_slopes_scale_glm.h): kernels for the one-wavefront geometries + registry entry
#include "models/hier_slopes_scale_glm.h"
#define WN_MODEL_ID 40
#define WN_MODEL_TAG hier_linear_regression_slopes_sigma
#define WN_MODEL_TYPE wn::HierLinearRegressionSlopesSigmaModel
#include "wn_kernels.inc"
