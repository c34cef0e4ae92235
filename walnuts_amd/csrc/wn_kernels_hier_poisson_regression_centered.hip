// the hier_poisson_regression_centered device model (models/hier_glm.h): kernels for the one-wavefront geometries + registry entry
#include "models/hier_glm.h"
#define WN_MODEL_ID 28
#define WN_MODEL_TAG hier_poisson_regression_centered
#define WN_MODEL_TYPE wn::HierPoissonRegressionCenteredModel
#include "wn_kernels.inc"
