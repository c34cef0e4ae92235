// the poisson_regression device model (models/glm.h): kernels for the one-wavefront geometries + registry entry
#include "models/glm.h"
#define WN_MODEL_ID 24
#define WN_MODEL_TAG poisson_regression
#define WN_MODEL_TYPE wn::PoissonRegressionModel
#include "wn_kernels.inc"
