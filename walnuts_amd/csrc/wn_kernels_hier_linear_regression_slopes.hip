// the hier_linear_regression_slopes device model (models/hier_slopes_glm.h): kernels for the one-wavefront geometries + registry entry
#include "models/hier_slopes_glm.h"
#define WN_MODEL_ID 32
#define WN_MODEL_TAG hier_linear_regression_slopes
#define WN_MODEL_TYPE wn::HierLinearRegressionSlopesModel
#include "wn_kernels.inc"
