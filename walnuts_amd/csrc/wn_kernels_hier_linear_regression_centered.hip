// the hier_linear_regression_centered device model (models/hier_glm.h): kernels for the one-wavefront geometries + registry entry
#include "models/hier_glm.h"
#define WN_MODEL_ID 17
#define WN_MODEL_TAG hier_linear_regression_centered
#define WN_MODEL_TYPE wn::HierLinearRegressionCenteredModel
#include "wn_kernels.inc"
