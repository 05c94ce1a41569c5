// dev.cpp -- kernel-variant switch table behind opk_dev_set / opk::dev_switch (common.h).
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

#include "../common.h"
#include "opk.h"

namespace opk {

namespace {
std::mutex g_mu;
std::map<std::string, int>& table()
{
    static std::map<std::string, int> t;
    return t;
}
}  // namespace

int dev_switch(const char* key, int dflt)
{
    std::lock_guard<std::mutex> lock(g_mu);
    const auto it = table().find(key);
    return it == table().end() ? dflt : it->second;
}

namespace {
thread_local LaunchLog* t_log = nullptr;
// the log behind opk_launch_log_begin / _end: one per thread, attached between the two calls
thread_local LaunchLog t_own_log;
}

void attach_launch_log(LaunchLog* log) { t_log = log; }
LaunchLog* launch_log() { return t_log; }

void note_launch(const char* fmt, ...)
{
    if (!t_log) return;
    char buf[160];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    t_log->lines.push_back(t_log->layer + "\t" + buf);
}

}  // namespace opk

extern "C" int opk_dev_set(const char* key, int value, int reset)
{
    if (!key) {
        opk::set_error("opk_dev_set: NULL key");
        return 1;
    }
    std::lock_guard<std::mutex> lock(opk::g_mu);
    if (reset)
        opk::table().erase(key);
    else
        opk::table()[key] = value;
    return 0;
}

extern "C" int opk_launch_log_begin(void)
{
    opk::t_own_log.layer.clear();
    opk::t_own_log.lines.clear();
    opk::attach_launch_log(&opk::t_own_log);
    return 0;
}

extern "C" int opk_launch_log_end(char* buf, size_t size, size_t* needed)
{
    if (!needed) {
        opk::set_error("opk_launch_log_end: NULL needed");
        return 1;
    }
    if (opk::launch_log() == &opk::t_own_log) opk::attach_launch_log(nullptr);
    std::string text;
    for (const auto& l : opk::t_own_log.lines) text += l + "\n";
    *needed = text.size() + 1;
    if (buf && size >= *needed) std::memcpy(buf, text.c_str(), text.size() + 1);
    return 0;
}
