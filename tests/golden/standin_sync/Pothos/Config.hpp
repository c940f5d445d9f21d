// Stand-in for <Pothos/Config.hpp>: test infrastructure of this project, written new, not PothosCore.  digital/FrameHelper.hpp of the
// reference includes this header and uses nothing of it.
#pragma once
