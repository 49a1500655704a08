/* compat include tree: a reference-style back end (#include <ais/ais_decode.h>) gets the host message layer of the GPU
 * AIS stage; ais_decode_on_events() takes the place of ais_decode_on_pcm(). */
#pragma once
#include "../../mfm_ais.h"
