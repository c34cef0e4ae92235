// the hier_poisson_regression device model (models/hier_glm.h): kernels for the one-wavefront geometries + registry entry
#include "models/hier_glm.h"
#define WN_MODEL_ID 27
#define WN_MODEL_TAG hier_poisson_regression
#define WN_MODEL_TYPE wn::HierPoissonRegressionModel
#include "wn_kernels.inc"
