// Limits of an overlap-save plan that its kernels (osm_chunk.hpp, also in run-time compiled
// sources) and its host geometry (osm_geo.hpp) share.  Nothing but constants.
#pragma once

#define BBT_MAX_CHUNK 16        // block descriptors one launch holds (OsmChunk::b)
#define BBT_MAX_LANES 8         // internal streams of a plan, each with its own work buffer
