// Stand-in for <Poco/Logger.h>: test infrastructure of this project, written new, not Poco.  utility/WaveTrigger.cpp of the reference
// logs one kind of line, a dropped buffer or packet; the stand-in counts them for the driver of tests/golden/make_trigger_golden.py.
#pragma once
#include <string>

namespace Poco {

class Logger {
public:
    static Logger &get(const std::string &)
    {
        static Logger l;
        return l;
    }
    template <typename... A> void error(const std::string &, A &&...) { errors++; }
    int errors = 0;
};

}  // namespace Poco
