// the hier_poisson_regression_slopes device model (models/hier_slopes_glm.h): kernels for the one-wavefront geometries + registry entry
#include "models/hier_slopes_glm.h"
#define WN_MODEL_ID 34
#define WN_MODEL_TAG hier_poisson_regression_slopes
#define WN_MODEL_TYPE wn::HierPoissonRegressionSlopesModel
#include "wn_kernels.inc"
